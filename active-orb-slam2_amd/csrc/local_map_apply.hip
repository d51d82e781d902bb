// aos2_local_map_apply (include/aos2.h): one keyframe's changes applied to the graph that an
// aos2_local_map handle keeps in HBM, without the graph crossing PCIe again.  The delta names the rows that change and carries
// their new content; the new arrays are built from the current device block and the uploaded delta into the handle's SECOND
// block, and the handle then points at that one.  The kernels of csrc/local_map.hip and csrc/kf_culling.hip keep reading exact
// CSR arrays through LmGraphDev / KfcGraph.  Integer and byte moves only (the two float arrays of the view move as 32-bit words).
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

// one CSR family rebuilt by the scan: its rows before and after, the delta's rows, the entries and the array parallel to them
struct LmaFam {
    int n_rows, n_old, n_d;
    const int32_t *old_off, *d_row, *d_off;
    int32_t *new_off, *totals;
    const int32_t *old_flat, *d_flat;
    int32_t *new_flat;
    const int32_t *old_idx, *d_idx;   // obs_idx; NULL = none
    int32_t *new_idx;
};
// the per-row scalars: of a point with family 0, of a keyframe's links with family 1 (th / flags NULL = no view)
struct LmaScalars {
    const uint8_t *old_point_bad, *d_point_bad, *old_kf_bad, *d_kf_bad, *old_flags, *d_flags;
    uint8_t *new_point_bad, *new_kf_bad, *new_flags;
    const int32_t *old_point_nobs, *d_point_nobs, *old_best, *d_best, *old_parent, *d_parent;
    int32_t *new_point_nobs, *new_best, *new_parent;
    const uint32_t *old_th, *d_th;
    uint32_t *new_th;
};
struct LmaArgs {
    LmaFam f[2];
    LmaScalars s;
    int tile;
};
struct LmaMatch {
    int n_rows, n_old, n_d, n_mp_old, s0;   // s0: the delta slot of the first appended keyframe
    const int32_t *old_off, *d_row, *d_off, *old_mp, *d_mp;
    int32_t *new_off, *new_mp;
    const uint8_t *old_octave, *d_octave, *old_stereo, *d_stereo;   // NULL = no view
    uint8_t *new_octave, *new_stereo;
    const uint32_t *old_depth, *d_depth;
    uint32_t *new_depth;
};

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
    const LmaScalars &S = A.s;
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
            if (slot >= 0) len = F.d_off[slot + 1] - F.d_off[slot];
            else if (old) len = F.old_off[r + 1] - F.old_off[r];
            if (fam == 0) {   // an appended row that is not named: the empty slot of the table
                S.new_point_bad[r] = slot >= 0 ? S.d_point_bad[slot] : (old ? S.old_point_bad[r] : (uint8_t)1);
                S.new_point_nobs[r] = slot >= 0 ? S.d_point_nobs[slot] : (old ? S.old_point_nobs[r] : 0);
            } else {
                S.new_kf_bad[r] = slot >= 0 ? S.d_kf_bad[slot] : (old ? S.old_kf_bad[r] : (uint8_t)1);
                S.new_parent[r] = slot >= 0 ? S.d_parent[slot] : (old ? S.old_parent[r] : -1);
                for (int j = 0; j < kLmNeighbours; ++j)
                    S.new_best[(size_t)r * kLmNeighbours + j] = slot >= 0 ? S.d_best[(size_t)slot * kLmNeighbours + j]
                                                                          : (old ? S.old_best[(size_t)r * kLmNeighbours + j] : -1);
                if (S.new_th) {
                    S.new_th[r] = slot >= 0 ? S.d_th[slot] : (old ? S.old_th[r] : 0u);
                    S.new_flags[r] = slot >= 0 ? S.d_flags[slot] : (old ? S.old_flags[r] : (uint8_t)0);
                }
            }
        }
        int total;
        const int ex = block_excl_scan_i32<kRT>(len, s_wsum, total);
        if (in) F.new_off[r] = run + ex;
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
    if (tid == 0) F.new_off[F.n_rows] = run;
}

__global__ __launch_bounds__(kRT) void k_lma_add(LmaArgs A)
{
    const LmaFam &F = A.f[blockIdx.y];
    const int stride = gridDim.x * kRT;
    for (int r = blockIdx.x * kRT + threadIdx.x; r < F.n_rows; r += stride) F.new_off[r] += F.totals[r / A.tile];
}

__global__ __launch_bounds__(kRT) void k_lma_copy(LmaArgs A)
{
    const LmaFam &F = A.f[blockIdx.y];
    const int sub = threadIdx.x % kRowLanes, stride = gridDim.x * (kRT / kRowLanes);
    for (int r = blockIdx.x * (kRT / kRowLanes) + threadIdx.x / kRowLanes; r < F.n_rows; r += stride) {
        const int d0 = F.new_off[r], len = F.new_off[r + 1] - d0;
        if (len <= 0) continue;
        const int slot = lma_slot(F.d_row, F.n_d, r);
        if (slot < 0 && r >= F.n_old) continue;   // (an appended row that is not named is empty: never reached)
        const int s0 = slot >= 0 ? F.d_off[slot] : F.old_off[r];
        const int32_t *src = (slot >= 0 ? F.d_flat : F.old_flat) + s0;
        const int32_t *isrc = F.new_idx ? (slot >= 0 ? F.d_idx : F.old_idx) + s0 : nullptr;
        for (int j = sub; j < len; j += kRowLanes) {
            F.new_flat[d0 + j] = src[j];
            if (isrc) F.new_idx[d0 + j] = isrc[j];
        }
    }
}

// workgroup r of n_rows + 1: offset r, and (r < n_rows) the entries of keyframe r
__global__ __launch_bounds__(kRT) void k_lma_matches(LmaMatch M)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    // rows up to the old count keep their offsets; the appended rows are the tail of the delta's rows, in order
    const int d0 = r <= M.n_old ? M.old_off[r] : M.n_mp_old + (M.d_off[M.s0 + (r - M.n_old)] - M.d_off[M.s0]);
    if (tid == 0) M.new_off[r] = d0;
    if (r >= M.n_rows) return;
    const int d1 = r + 1 <= M.n_old ? M.old_off[r + 1] : M.n_mp_old + (M.d_off[M.s0 + (r + 1 - M.n_old)] - M.d_off[M.s0]);
    const int slot = lma_slot(M.d_row, M.n_d, r);
    if (slot < 0 && r >= M.n_old) return;   // (an appended keyframe is always named)
    const int s0 = slot >= 0 ? M.d_off[slot] : M.old_off[r];
    const int len = min(d1 - d0, slot >= 0 ? M.d_off[slot + 1] - s0 : M.old_off[r + 1] - s0);   // (equal: the host has checked)
    const bool d = slot >= 0;
    for (int j = tid; j < len; j += kRT) {
        M.new_mp[d0 + j] = (d ? M.d_mp : M.old_mp)[s0 + j];
        if (M.new_octave) {
            M.new_octave[d0 + j] = (d ? M.d_octave : M.old_octave)[s0 + j];
            M.new_depth[d0 + j] = (d ? M.d_depth : M.old_depth)[s0 + j];
            M.new_stereo[d0 + j] = (d ? M.d_stereo : M.old_stereo)[s0 + j];
        }
    }
}

bool fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
bool fail(const char *fmt, ...)
{
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    set_error("local map delta: %s", msg);
    return true;
}

// a row list: strictly ascending, inside [0, n_new)
bool bad_row_list(const int32_t *row, int n, int n_new, const char *what)
{
    if (n < 0) return fail("%s holds %d rows", what, n);
    if (n > 0 && !row) return fail("%s is NULL", what);
    for (int i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= n_new) return fail("%s[%d] = %d is outside [0, %d)", what, i, row[i], n_new);
        if (i && row[i] <= row[i - 1]) return fail("%s is not strictly ascending at %d", what, i);
    }
    return false;
}

bool bad_delta_off(const int32_t *off, int n, const char *what)
{
    if (n == 0) return false;   // (no rows: the array is not read)
    if (!off) return fail("%s is NULL", what);
    if (off[0] != 0) return fail("%s starts at %d", what, off[0]);
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail("%s decreases at row %d", what, i);
    return false;
}

bool bad_values(const int32_t *v, int64_t n, int lo, int hi, const char *what)
{
    if (n > 0 && !v) return fail("%s is NULL", what);
    for (int64_t i = 0; i < n; ++i)
        if (v[i] < lo || v[i] >= hi) return fail("%s[%lld] = %d is outside [%d, %d)", what, (long long)i, v[i], lo, hi);
    return false;
}

// the entry counts of the three arrays after the delta, from the row lengths the handle keeps
struct NewCounts {
    int64_t n_obs, n_mp, n_child;
};
NewCounts new_counts(const aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    NewCounts c = {h->n_obs, h->n_mp, h->n_child};
    for (int i = 0; i < d->n_point_rows; ++i) {
        const int r = d->point_row[i];
        c.n_obs += (d->obs_off[i + 1] - d->obs_off[i]) - (r < h->n_points ? h->row_obs[r] : 0);
    }
    for (int i = 0; i < d->n_kf_mp_rows; ++i)
        if (d->kf_mp_row[i] >= h->n_kfs) c.n_mp += d->kf_mp_off[i + 1] - d->kf_mp_off[i];
    for (int i = 0; i < d->n_kf_link_rows; ++i) {
        const int r = d->kf_link_row[i];
        c.n_child += (d->kf_child_off[i + 1] - d->kf_child_off[i]) - (r < h->n_kfs ? h->row_child[r] : 0);
    }
    return c;
}

// the counts and row lengths of the handle after a delta that has been applied, in O(delta)
void commit_counts(aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    const NewCounts c = new_counts(h, d);
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
    h->n_obs = c.n_obs; h->n_mp = c.n_mp; h->n_child = c.n_child;
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

// the delta's arrays on the device (and, while they are filled, in the page-locked staging buffer)
struct DeltaDev {
    const int32_t *point_row, *point_nobs, *obs_off, *obs_kf, *obs_idx, *kf_mp_row, *kf_mp_off, *kf_mp, *kf_link_row, *kf_best, *kf_child_off,
        *kf_child, *kf_parent;
    const uint8_t *point_bad, *kf_bad, *kf_stereo, *kf_flags;
    const int8_t *kf_octave;
    const float *kf_depth, *kf_th_depth;
};

template <class T>
void stage(const T *dst, const T *src, size_t n)
{
    if (n) memcpy(const_cast<T *>(dst), src, n * sizeof(T));
}

template <class T>
T *rw(const T *p) { return const_cast<T *>(p); }
inline const uint32_t *words(const float *p) { return reinterpret_cast<const uint32_t *>(p); }

int apply_device(aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    KfcState &K = h->kfc;
    const bool view = K.has_view;
    const int np = d->n_points, nk = d->n_keyframes, np0 = h->n_points, nk0 = h->n_kfs;
    const int npr = d->n_point_rows, nmr = d->n_kf_mp_rows, nlr = d->n_kf_link_rows;
    const NewCounts c = new_counts(h, d);
    const size_t d_obs = npr ? d->obs_off[npr] : 0, d_mp = nmr ? d->kf_mp_off[nmr] : 0, d_child = nlr ? d->kf_child_off[nlr] : 0;
    const int tile = h->apply_tile > 0 ? h->apply_tile : kTileDefault;
    const int tiles0 = (int)(((int64_t)np + tile - 1) / tile), tiles1 = (int)(((int64_t)nk + tile - 1) / tile);

    int st;
    if ((st = bind_device(h->device))) return st;
    AOS2_HIP_CHECK(hipDeviceSynchronize());   // (the ordering contract of aos2_local_map_set: calls enqueued before this one are done)
    if (!h->stream && (st = stream_create(&h->stream, false))) return st;
    if (!h->ap_ev0) {
        AOS2_HIP_CHECK(hipEventCreate(&h->ap_ev0));
        AOS2_HIP_CHECK(hipEventCreate(&h->ap_ev1));
    }
    h->apply_timed = false;

    // the new block: the graph, the view, and behind them the totals of the scan (not part of what a download copies)
    LmGraphDev G = {};
    KfcGraph V = {};
    int32_t *totals0, *totals1;
    G.n_points = np; G.n_kfs = nk;
    Regions<19> R;
    R.add(G.point_bad, np); R.add(G.kf_bad, nk); R.add(G.point_nobs, np); R.add(G.obs_off, (size_t)np + 1); R.add(G.obs_kf, c.n_obs);
    R.add(G.kf_mp_off, (size_t)nk + 1); R.add(G.kf_mp, c.n_mp); R.add(G.kf_best, (size_t)nk * kLmNeighbours);
    R.add(G.kf_child_off, (size_t)nk + 1); R.add(G.kf_child, c.n_child); R.add(G.kf_parent, nk);
    if (view) {
        R.add(V.obs_idx, c.n_obs); R.add(V.kf_octave, c.n_mp); R.add(V.kf_depth, c.n_mp); R.add(V.kf_stereo, c.n_mp);
        R.add(V.kf_th_depth, nk); R.add(V.kf_flags, nk);
    }
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
    DeltaDev D = {};
    Regions<20> Q;
    Q.add(D.point_row, npr); Q.add(D.point_bad, npr); Q.add(D.point_nobs, npr); Q.add(D.obs_off, (size_t)npr + 1); Q.add(D.obs_kf, d_obs);
    Q.add(D.kf_mp_row, nmr); Q.add(D.kf_mp_off, (size_t)nmr + 1); Q.add(D.kf_mp, d_mp);
    Q.add(D.kf_link_row, nlr); Q.add(D.kf_bad, nlr); Q.add(D.kf_best, (size_t)nlr * kLmNeighbours); Q.add(D.kf_child_off, (size_t)nlr + 1);
    Q.add(D.kf_child, d_child); Q.add(D.kf_parent, nlr);
    if (view) {
        Q.add(D.obs_idx, d_obs); Q.add(D.kf_octave, d_mp); Q.add(D.kf_depth, d_mp); Q.add(D.kf_stereo, d_mp);
        Q.add(D.kf_th_depth, nlr); Q.add(D.kf_flags, nlr);
    }
    const size_t d_bytes = Q.bytes();
    if ((st = h->delta_stage.alloc(d_bytes + 256))) return st;
    if ((st = h->d_delta.alloc(d_bytes + 256))) return st;
    Q.bind(h->delta_stage.p);
    const int32_t zero = 0;
    stage(D.point_row, d->point_row, npr); stage(D.point_bad, d->point_bad, npr); stage(D.point_nobs, d->point_nobs, npr);
    stage(D.obs_off, npr ? d->obs_off : &zero, (size_t)npr + 1); stage(D.obs_kf, d->obs_kf, d_obs);
    stage(D.kf_mp_row, d->kf_mp_row, nmr); stage(D.kf_mp_off, nmr ? d->kf_mp_off : &zero, (size_t)nmr + 1); stage(D.kf_mp, d->kf_mp, d_mp);
    stage(D.kf_link_row, d->kf_link_row, nlr); stage(D.kf_bad, d->kf_bad, nlr); stage(D.kf_best, d->kf_best, (size_t)nlr * kLmNeighbours);
    stage(D.kf_child_off, nlr ? d->kf_child_off : &zero, (size_t)nlr + 1); stage(D.kf_child, d->kf_child, d_child);
    stage(D.kf_parent, d->kf_parent, nlr);
    for (int i = 0; i < nlr; ++i)   // set<KeyFrame*> spChilds: ascending row, as aos2_local_map_set stores it
        std::sort(rw(D.kf_child) + d->kf_child_off[i], rw(D.kf_child) + d->kf_child_off[i + 1]);
    if (view) {
        const aos2_kf_culling_view_t *v = d->view;
        stage(D.obs_idx, v->obs_idx, d_obs); stage(D.kf_octave, v->kf_octave, d_mp); stage(D.kf_depth, v->kf_depth, d_mp);
        stage(D.kf_stereo, v->kf_stereo, d_mp); stage(D.kf_th_depth, v->kf_th_depth, nlr); stage(D.kf_flags, v->kf_flags, nlr);
    }
    hipStream_t q = h->stream;
    AOS2_HIP_CHECK(hipEventRecord(h->ap_ev0, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(h->d_delta.p, h->delta_stage.p, d_bytes, hipMemcpyHostToDevice, q));
    Q.bind(h->d_delta.p);

    const LmGraphDev &O = h->G;
    const KfcGraph &OV = K.V;
    LmaArgs A = {};
    A.tile = tile;
    A.f[0] = LmaFam{np, np0, npr, O.obs_off, D.point_row, D.obs_off, rw(G.obs_off), totals0, O.obs_kf, D.obs_kf, rw(G.obs_kf),
                    view ? OV.obs_idx : nullptr, view ? D.obs_idx : nullptr, view ? rw(V.obs_idx) : nullptr};
    A.f[1] = LmaFam{nk, nk0, nlr, O.kf_child_off, D.kf_link_row, D.kf_child_off, rw(G.kf_child_off), totals1, O.kf_child, D.kf_child,
                    rw(G.kf_child), nullptr, nullptr, nullptr};
    LmaScalars &S = A.s;
    S.old_point_bad = O.point_bad; S.d_point_bad = D.point_bad; S.new_point_bad = rw(G.point_bad);
    S.old_point_nobs = O.point_nobs; S.d_point_nobs = D.point_nobs; S.new_point_nobs = rw(G.point_nobs);
    S.old_kf_bad = O.kf_bad; S.d_kf_bad = D.kf_bad; S.new_kf_bad = rw(G.kf_bad);
    S.old_best = O.kf_best; S.d_best = D.kf_best; S.new_best = rw(G.kf_best);
    S.old_parent = O.kf_parent; S.d_parent = D.kf_parent; S.new_parent = rw(G.kf_parent);
    if (view) {
        S.old_th = words(OV.kf_th_depth); S.d_th = words(D.kf_th_depth); S.new_th = rw(words(V.kf_th_depth));
        S.old_flags = OV.kf_flags; S.d_flags = D.kf_flags; S.new_flags = rw(V.kf_flags);
    }
    LmaMatch M = {};
    M.n_rows = nk; M.n_old = nk0; M.n_d = nmr; M.n_mp_old = (int)h->n_mp; M.s0 = nmr - (nk - nk0);
    M.old_off = O.kf_mp_off; M.d_row = D.kf_mp_row; M.d_off = D.kf_mp_off; M.old_mp = O.kf_mp; M.d_mp = D.kf_mp;
    M.new_off = rw(G.kf_mp_off); M.new_mp = rw(G.kf_mp);
    if (view) {
        M.old_octave = reinterpret_cast<const uint8_t *>(OV.kf_octave); M.d_octave = reinterpret_cast<const uint8_t *>(D.kf_octave);
        M.new_octave = reinterpret_cast<uint8_t *>(rw(V.kf_octave));
        M.old_depth = words(OV.kf_depth); M.d_depth = words(D.kf_depth); M.new_depth = rw(words(V.kf_depth));
        M.old_stereo = OV.kf_stereo; M.d_stereo = D.kf_stereo; M.new_stereo = rw(V.kf_stereo);
    }
    const int max_rows = std::max(np, nk), max_tiles = std::max(std::max(tiles0, tiles1), 1);
    const int add_blocks = std::max(1, std::min(2048, (max_rows + kRT - 1) / kRT));
    const int copy_rows = kRT / kRowLanes, copy_blocks = std::max(1, std::min(8192, (max_rows + copy_rows - 1) / copy_rows));
    hipLaunchKernelGGL(k_lma_rows, dim3(max_tiles, 2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_totals, dim3(2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_add, dim3(add_blocks, 2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_copy, dim3(copy_blocks, 2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_matches, dim3(nk + 1), dim3(kRT), 0, q, M);
    AOS2_HIP_CHECK(hipGetLastError());
    AOS2_HIP_CHECK(hipEventRecord(h->ap_ev1, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    // the new block is complete: it becomes the handle's, the previous one the spare
    std::swap(h->d_graph, h->d_spare);
    h->G = G;
    if (view) K.V = V;
    h->block_bytes = block_bytes;
    h->host_stale = true;
    h->apply_timed = true;
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
    h->apply_timed = false;
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
    if (np < np0 || nk < nk0) {
        fail("%d points and %d keyframes are fewer than the handle's %d and %d (rows only get appended)", np, nk, np0, nk0);
        return AOS2_ERR_ARG;
    }
    if (np > kMaxRows || nk > kMaxRows) {
        fail("more than 2^30 rows");
        return AOS2_ERR_ARG;
    }
    if (bad_row_list(d->point_row, npr, np, "point_row") || bad_row_list(d->kf_mp_row, nmr, nk, "kf_mp_row") ||
        bad_row_list(d->kf_link_row, nlr, nk, "kf_link_row"))
        return AOS2_ERR_ARG;
    // (ascending and inside the count: the appended keyframes are all named exactly when the tail of the list holds that many)
    const int n_app = nk - nk0;
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *row = pass ? d->kf_link_row : d->kf_mp_row;
        const int n = pass ? nlr : nmr;
        if (n_app > 0 && (n < n_app || row[n - n_app] != nk0)) {
            fail("an appended keyframe is missing from %s", pass ? "kf_link_row" : "kf_mp_row");
            return AOS2_ERR_ARG;
        }
    }
    if ((npr > 0 && (!d->point_bad || !d->point_nobs)) || (nlr > 0 && (!d->kf_bad || !d->kf_best || !d->kf_parent))) {
        fail("an array is NULL");
        return AOS2_ERR_ARG;
    }
    if (bad_delta_off(d->obs_off, npr, "obs_off") || bad_delta_off(d->kf_mp_off, nmr, "kf_mp_off") ||
        bad_delta_off(d->kf_child_off, nlr, "kf_child_off"))
        return AOS2_ERR_ARG;
    const int64_t d_obs = npr ? d->obs_off[npr] : 0, d_mp = nmr ? d->kf_mp_off[nmr] : 0, d_child = nlr ? d->kf_child_off[nlr] : 0;
    if (bad_values(d->obs_kf, d_obs, 0, nk, "obs_kf") || bad_values(d->kf_mp, d_mp, -1, np, "kf_mp") ||
        bad_values(d->kf_best, (int64_t)nlr * kLmNeighbours, -1, nk, "kf_best") || bad_values(d->kf_child, d_child, 0, nk, "kf_child") ||
        bad_values(d->kf_parent, nlr, -1, nk, "kf_parent"))
        return AOS2_ERR_ARG;
    std::vector<int32_t> row;
    for (int i = 0; i < npr; ++i) {   // a keyframe at most once per point
        row.assign(d->obs_kf + d->obs_off[i], d->obs_kf + d->obs_off[i + 1]);
        std::sort(row.begin(), row.end());
        const auto twice = std::adjacent_find(row.begin(), row.end());
        if (twice != row.end()) {
            fail("point %d lists keyframe %d twice", d->point_row[i], *twice);
            return AOS2_ERR_ARG;
        }
    }
    for (int i = 0; i < nmr; ++i) {   // Frame::N of a keyframe never changes
        const int r = d->kf_mp_row[i], len = d->kf_mp_off[i + 1] - d->kf_mp_off[i];
        if (r < nk0 && len != h->row_feat[r]) {
            fail("the match row of keyframe %d holds %d entries, the keyframe has %d features", r, len, h->row_feat[r]);
            return AOS2_ERR_ARG;
        }
    }
    const aos2_kf_culling_view_t *v = d->view;
    if ((v != nullptr) != h->kfc.has_view) {
        fail(v ? "a view is given, the handle holds none" : "the handle holds a culling view, the delta carries none");
        return AOS2_ERR_ARG;
    }
    if (v) {
        if ((d_obs > 0 && !v->obs_idx) || (d_mp > 0 && (!v->kf_octave || !v->kf_depth || !v->kf_stereo)) ||
            (nlr > 0 && (!v->kf_th_depth || !v->kf_flags))) {
            fail("an array of the view is NULL");
            return AOS2_ERR_ARG;
        }
        for (int i = 0; i < npr; ++i)
            for (int e = d->obs_off[i]; e < d->obs_off[i + 1]; ++e) {
                const int kf = d->obs_kf[e];
                const int slot = nmr - (nk - kf);   // (of an appended keyframe: they are the tail of kf_mp_row)
                const int nf = kf < nk0 ? h->row_feat[kf] : d->kf_mp_off[slot + 1] - d->kf_mp_off[slot];
                if (v->obs_idx[e] < 0 || v->obs_idx[e] >= nf) {
                    fail("obs_idx[%d] = %d of point %d is outside the %d features of keyframe %d", e, v->obs_idx[e], d->point_row[i], nf, kf);
                    return AOS2_ERR_ARG;
                }
            }
    }
    const NewCounts c = new_counts(h, d);
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (c.n_obs > lim || c.n_mp > lim || c.n_child > lim) {
        fail("more than 2^31 - 1 entries in an array");
        return AOS2_ERR_ARG;
    }
    return AOS2_OK;
}

void local_map_apply_host(aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    KfcState &K = h->kfc;
    const aos2_kf_culling_view_t *v = K.has_view ? d->view : nullptr;
    const int np = d->n_points, nk = d->n_keyframes, np0 = h->n_points, nk0 = h->n_kfs;
    const int npr = d->n_point_rows, nmr = d->n_kf_mp_rows, nlr = d->n_kf_link_rows;
    std::vector<int32_t> off;
    {   // observations over points
        const std::vector<RowSrc> plan = plan_rows(np, np0, h->obs_off, npr, d->point_row, d->obs_off, off);
        move_rows(plan, off, h->obs_kf, d->obs_kf);
        if (v) move_rows(plan, off, K.obs_idx, v->obs_idx);
        h->obs_off.swap(off);
    }
    {   // matches over keyframes
        const std::vector<RowSrc> plan = plan_rows(nk, nk0, h->kf_mp_off, nmr, d->kf_mp_row, d->kf_mp_off, off);
        move_rows(plan, off, h->kf_mp, d->kf_mp);
        if (v) {
            move_rows(plan, off, K.kf_octave, v->kf_octave);
            move_rows(plan, off, K.kf_depth, v->kf_depth);
            move_rows(plan, off, K.kf_stereo, v->kf_stereo);
        }
        h->kf_mp_off.swap(off);
    }
    {   // children over keyframes, a named row in ascending row
        const std::vector<RowSrc> plan = plan_rows(nk, nk0, h->kf_child_off, nlr, d->kf_link_row, d->kf_child_off, off);
        move_rows(plan, off, h->kf_child, d->kf_child);
        h->kf_child_off.swap(off);
        for (int i = 0; i < nlr; ++i) {
            const int r = d->kf_link_row[i];
            std::sort(h->kf_child.begin() + h->kf_child_off[r], h->kf_child.begin() + h->kf_child_off[r + 1]);
        }
    }
    put_rows<uint8_t>(h->point_bad, np, 1, npr, d->point_row, d->point_bad);   // an appended row that is not named: the empty slot
    put_rows<int32_t>(h->point_nobs, np, 0, npr, d->point_row, d->point_nobs);
    put_rows<uint8_t>(h->kf_bad, nk, 1, nlr, d->kf_link_row, d->kf_bad);
    put_rows<int32_t>(h->kf_best, nk, -1, nlr, d->kf_link_row, d->kf_best, kLmNeighbours);
    put_rows<int32_t>(h->kf_parent, nk, -1, nlr, d->kf_link_row, d->kf_parent);
    if (v) {
        put_rows<float>(K.kf_th_depth, nk, 0.f, nlr, d->kf_link_row, v->kf_th_depth);
        put_rows<uint8_t>(K.kf_flags, nk, 0, nlr, d->kf_link_row, v->kf_flags);
    }
    commit_counts(h, d);
}

void local_map_recount(aos2_local_map *h)
{
    const int np = h->n_points, nk = h->n_kfs;
    h->row_obs.resize(np);
    h->row_feat.resize(nk);
    h->row_child.resize(nk);
    for (int p = 0; p < np; ++p) h->row_obs[p] = h->obs_off[p + 1] - h->obs_off[p];
    for (int k = 0; k < nk; ++k) {
        h->row_feat[k] = h->kf_mp_off[k + 1] - h->kf_mp_off[k];
        h->row_child[k] = h->kf_child_off[k + 1] - h->kf_child_off[k];
    }
    h->n_obs = h->obs_off[np];
    h->n_mp = h->kf_mp_off[nk];
    h->n_child = h->kf_child_off[nk];
}

int local_map_refresh_host(aos2_local_map *h)
{
    if (!h->host_stale) return AOS2_OK;
    if (int st = bind_device(h->device)) return st;
    std::vector<uint8_t> buf(h->block_bytes + 1);
    AOS2_HIP_CHECK(hipMemcpy(buf.data(), h->d_graph.p, h->block_bytes, hipMemcpyDeviceToHost));   // the one download
    auto take = [&](auto &vec, const auto *dev, size_t n) {
        vec.resize(n);
        if (n) memcpy(vec.data(), buf.data() + (reinterpret_cast<const uint8_t *>(dev) - h->d_graph.p), n * sizeof(vec[0]));
    };
    const size_t np = (size_t)h->n_points, nk = (size_t)h->n_kfs, n_obs = (size_t)h->n_obs, n_mp = (size_t)h->n_mp;
    const LmGraphDev &G = h->G;
    take(h->point_bad, G.point_bad, np); take(h->point_nobs, G.point_nobs, np); take(h->obs_off, G.obs_off, np + 1);
    take(h->obs_kf, G.obs_kf, n_obs); take(h->kf_bad, G.kf_bad, nk); take(h->kf_mp_off, G.kf_mp_off, nk + 1); take(h->kf_mp, G.kf_mp, n_mp);
    take(h->kf_best, G.kf_best, nk * kLmNeighbours); take(h->kf_child_off, G.kf_child_off, nk + 1);
    take(h->kf_child, G.kf_child, (size_t)h->n_child); take(h->kf_parent, G.kf_parent, nk);
    KfcState &K = h->kfc;
    if (K.has_view) {
        const KfcGraph &V = K.V;
        take(K.obs_idx, V.obs_idx, n_obs); take(K.kf_octave, V.kf_octave, n_mp); take(K.kf_depth, V.kf_depth, n_mp);
        take(K.kf_stereo, V.kf_stereo, n_mp); take(K.kf_th_depth, V.kf_th_depth, nk); take(K.kf_flags, V.kf_flags, nk);
    }
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
        float ms = -1.f;
        if (!h->apply_timed || hipEventSynchronize(h->ap_ev1) != hipSuccess || hipEventElapsedTime(&ms, h->ap_ev0, h->ap_ev1) != hipSuccess)
            ms = -1.f;
        *device_ms = ms;
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
