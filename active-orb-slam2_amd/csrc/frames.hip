// Device-resident frame batches (include/aos2.h: aos2_frames_*): lifetime, Frame::Frame, and the two searches of the per-frame
// tracking chain.  A batch holds B Frames whose members stay in HBM between the calls of the chain; every call is enqueued on the
// batch's own stream and returns without waiting.  The searches are built from the device routines of search_device.h, which the
// matcher's kernels share.  The keyframe work on resident batches is frames_keyframe.hip, PoseOptimization frames_pose.hip, the
// local map local_map.hip.
//
// Reference: Frame::Frame (src/Frame.cc:116-170), Tracking::TrackWithMotionModel (src/Tracking.cc:963-1027),
// Tracking::SearchLocalPoints (:1302-1352), ORBmatcher::SearchByProjection (src/ORBmatcher.cc:45-129, 1328-1470),
// Frame::isInFrustum (src/Frame.cc:298-354).
#include <algorithm>

#include "frames.h"
#include "search_device.h"

namespace aos2 {

// Frame::Frame after ExtractORB (:126-150): N, UndistortKeyPoints with zero distortion (mvKeysUn = mvKeys :436-442),
// ComputeStereoFromRGBD (:672-693), mvpMapPoints = NULL, mvbOutlier = false
// Frame::Frame after ExtractORB as ONE launch, one workgroup per frame: the members above, then
// Frame::AssignFeaturesToGrid (:259-274) on the coordinates just written
// (ur_in / dp_in, [batch][cap]: the stereo constructor's mvuRight / mvDepth, written by ComputeStereoMatches -- src/Frame.cc:57-113)
__global__ __launch_bounds__(256) void frames_build_kernel(FramesDev S, const float *__restrict__ depth, int dstride, size_t dimg_stride,
                                                           const float *__restrict__ ur_in, const float *__restrict__ dp_in)
{
    const int b = blockIdx.x;
    const size_t ob = (size_t)b * S.cap;
    const int n = S.n[b];
    for (int i = threadIdx.x; i < S.cap; i += 256) {
        const size_t o = ob + i;
        float x = 0, y = 0, ang = 0, ur = -1.0f, dp = -1.0f;
        int oct = 0;
        if (i < n) {
            const aos2_keypoint_t k = S.kps[o];
            x = k.x; y = k.y; ang = k.angle; oct = k.octave;
            float d = 0.f;
            if (depth) d = depth[(size_t)b * dimg_stride + (size_t)(int)y * dstride + (int)x];   // imDepth.at<float>(v, u) at mvKeys[i].pt (:678-683)
            if (S.has_dist) undistort_point(S.fx, S.fy, S.cx, S.cy, S.dist, x, y, x, y);   // mvKeysUn[i].pt (:433-461)
            if (d > 0) {
                dp = d;
                ur = __fsub_rn(x, __fdiv_rn(S.mbf, d));   // kpU.pt.x - mbf / d (:688)
            }
            if (ur_in) {
                ur = ur_in[o];
                dp = dp_in[o];
            }
        }
        S.kp_x[o] = x; S.kp_y[o] = y; S.kp_angle[o] = ang; S.kp_octave[o] = oct;
        S.u_right[o] = ur; S.depth[o] = dp;
        S.mp[o] = -1; S.mp_seen[o] = -1; S.mp_state[o] = 0; S.outlier[o] = 0;
    }
    __syncthreads();
    assign_grid_body(n, S.kp_x + ob, S.kp_y + ob, S.min_x, S.min_y, S.grid_w_inv, S.grid_h_inv,
                     S.grid_off + (size_t)b * (kFrGridCells + 1), S.grid_idx + ob);
}

__global__ __launch_bounds__(256) void frames_scan_slots_kernel(QuerySlot *__restrict__ slots, const int32_t *__restrict__ nq_of,
                                                                int nq_cap, int share, int32_t *__restrict__ overflow)
{
    scan_slots_body(slots, nq_of, nq_cap, share, overflow);
}

// ---- SearchByProjection(CurrentFrame, LastFrame, th, bMono) for the pairs (cur b, last b)
__device__ __forceinline__ ProjLastDev last_of(const FramesDev &cur, const FramesDev &last, const MapPointsDev &M, int b)
{
    ProjLastDev P;
    const size_t o = (size_t)b * last.cap;
    P.n_last = last.n[b];
    P.last_valid = nullptr;
    P.desc = M.desc;
    P.has_obs = M.has_obs;
    P.world_pos = M.pos;
    P.last_angle = last.kp_angle + o;
    P.last_octave = last.kp_octave + o;   // LastFrame.mvKeys[i].octave (:1360)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        P.Tcw[k] = cur.Tcw[(size_t)b * 16 + k];
        P.Tlw[k] = last.Tcw[(size_t)b * 16 + k];
    }
    P.fx = cur.fx; P.fy = cur.fy; P.cx = cur.cx; P.cy = cur.cy; P.mb = cur.mb; P.mbf = cur.mbf;
    P.mp_idx = last.mp + o;
    P.outlier = last.outlier + o;
    return P;
}

// a wave per query (4 waves per workgroup measured slower: 0.48 vs 0.43 ms for 256 frames)
// (a wave per query, one query per workgroup: four waves per workgroup were measured for the 540 k / 768 k workgroup grids of a
// 512-frame batch -- slower: 0.265 -> 0.286 and 0.204 -> 0.235 ms for the two fill kernels)
constexpr int kEntryWaves = 1;
__global__ __launch_bounds__(64 * kEntryWaves) void frames_last_entries_kernel(FramesDev cur, FramesDev last, MapPointsDev M, float th, int mono,
                                                                 QuerySlot *slots, Entry *pool, int32_t *overflow, int phase, QueryRec *rec)
{
    const int b = blockIdx.y, i = kEntryWaves * blockIdx.x + (threadIdx.x >> 6);
    if (phase != 2 && i >= last.n[b]) return;   // (the fill pass reads the slot first: 0 beyond the frame's features)
    const FrameDev F = frame_of(cur, b);
    const ProjLastDev P = last_of(cur, last, M, b);
    proj_last_entries_body(F, P, th, mono, slots + (size_t)b * last.cap, pool, overflow, 0, i, 0, phase, rec + (size_t)b * last.cap);
}

// counting pass of the candidate pool: one THREAD per query (a wave per query is 256 k one-wave workgroups for a batch of 256
// frames, most of their time dispatch)
__global__ __launch_bounds__(256) void frames_last_count_kernel(FramesDev cur, FramesDev last, MapPointsDev M, float th, int mono,
                                                               QuerySlot *slots, QueryRec *rec)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= last.n[b]) return;
    const FrameDev F = frame_of(cur, b);
    const ProjLastDev P = last_of(cur, last, M, b);
    proj_last_entries_body<true>(F, P, th, mono, slots + (size_t)b * last.cap, nullptr, nullptr, 0, i, 0, 1, rec + (size_t)b * last.cap);
}

// (four waves per SIMD -- 136 -> 128 registers for 40 bytes of scratch per lane: a 512-frame batch is 4096 waves, one round of the device
// instead of 1.33: 141 -> 93 us; the same for the local-points resolve, 72 -> 48 us)
// NT = 1024 for frames of more than 1536 queries (KITTI: 2000 features per frame): the fixed-point resolve keeps up to 3 queries per
// thread in registers; beyond that every pass walks the queries' entries in global memory -- 1.74 ms per 256 KITTI frames with 512
// threads (round 4: 20 x the per-frame time of the 1000-feature frames), the form below with 1024
template <int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void frames_last_resolve_kernel(FramesDev cur, FramesDev last, MapPointsDev M, int check_ori,
                                                                  const QuerySlot *__restrict__ slots, const Entry *__restrict__ pool,
                                                                  int32_t *match_f, uint32_t *bin_f, int32_t *nmatches, int32_t *choice,
                                                                  int32_t *nmatches_user)
{
    const int b = blockIdx.x;
    const FrameDev F = frame_of(cur, b);
    const ProjLastDev P = last_of(cur, last, M, b);
    proj_last_resolve_fix_body<NT>(F, P, check_ori, slots + (size_t)b * last.cap, pool, match_f + (size_t)b * cur.cap,
                                    bin_f + (size_t)b * cur.cap, nmatches + b, choice + (size_t)b * last.cap);
    __syncthreads();
    // CurrentFrame.mvpMapPoints[bestIdx2] = pMP (:1432), reset to NULL by the rotation check (:1459) -- same launch
    for (int j = threadIdx.x; j < cur.n[b]; j += NT) {
        const size_t o = (size_t)b * cur.cap + j;
        const int m = match_f[o];
        if (m >= 0) {
            const int row = last.mp[(size_t)b * last.cap + m];
            cur.mp[o] = row;
            cur.mp_state[o] = row < 0 ? 0 : (M.has_obs[row] ? 2 : 1);
        } else if (m == -2) {
            cur.mp[o] = -1;
            cur.mp_state[o] = 0;
        }
    }
    if (threadIdx.x == 0 && nmatches_user) nmatches_user[b] = nmatches[b];
}

// Tracking::TrackWithMotionModel :1008-1025 after PoseOptimization: an outlier loses its map point (which counts as
// seen in this frame: pMP->mnLastFrameSeen = mCurrentFrame.mnId, so SearchLocalPoints skips it)
__global__ __launch_bounds__(256) void frames_discard_kernel(FramesDev S)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S.n[b]) return;
    const size_t o = (size_t)b * S.cap + i;
    if (S.mp[o] >= 0 && S.outlier[o]) {
        S.mp_seen[o] = S.mp[o];
        S.mp[o] = -1;
        S.mp_state[o] = 0;
        S.outlier[o] = 0;
    }
}

// ---- Tracking::SearchLocalPoints (:1302-1352), first half: the map points already in the frame are marked as seen
// (:1305-1322), every other local map point goes through Frame::isInFrustum(pMP, 0.5) (src/Frame.cc:298-354).
// One workgroup per frame: the seen set is an LDS hash of the frame's map-point rows.
struct LocalDev {
    int n_local;                 // entries per frame
    const int32_t *local;        // [B][n_local] rows of the map-point table, -1 = none
    uint8_t *in_view, *has_obs;  // [B][n_local]
    float *proj_x, *proj_y, *proj_xr, *view_cos;
    int32_t *pred_level, *desc_idx;
};

__global__ __launch_bounds__(256) void frames_frustum_kernel(FramesDev S, MapPointsDev M, LocalDev L, float cos_limit)
{
    constexpr int HS = 16384;   // >= 2 x the (mp, mp_seen) entries of a frame with cap <= 4096 features
    __shared__ int32_t hs[HS];
    __shared__ float Rt[12], Ow[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < HS; i += 256) hs[i] = -1;
    if (tid < 12) Rt[tid] = S.Tcw[(size_t)b * 16 + tid];   // rows of [Rcw | tcw]
    __syncthreads();
    if (tid < 3) {   // mOw = -mRcw.t() * mtcw (Frame::UpdatePoseMatrices :251-257; cv::gemm: double accumulation)
        const double sacc = __dadd_rn(__dadd_rn(__dmul_rn((double)Rt[tid], (double)Rt[3]), __dmul_rn((double)Rt[4 + tid], (double)Rt[7])),
                                      __dmul_rn((double)Rt[8 + tid], (double)Rt[11]));
        Ow[tid] = (float)__dmul_rn(sacc, -1.0);
    }
    const size_t o = (size_t)b * S.cap;
    const int n = S.n[b];
    for (int i = tid; i < n; i += 256) {
        for (int pass = 0; pass < 2; ++pass) {
            const int row = pass == 0 ? S.mp[o + i] : S.mp_seen[o + i];
            if (row < 0) continue;
            unsigned h = ((unsigned)row * 2654435761u) >> 18;   // 14 bits
            for (;;) {
                const int prev = atomicCAS(&hs[h], -1, row);
                if (prev == -1 || prev == row) break;
                h = (h + 1) & (HS - 1);
            }
        }
    }
    __syncthreads();
    const float R[9] = {Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10]};
    const float t[3] = {Rt[3], Rt[7], Rt[11]};
    const size_t lo = (size_t)b * L.n_local;
    for (int q = tid; q < L.n_local; q += 256) {
        const int row = L.local[lo + q];
        uint8_t ok = 0, hobs = 0;
        float u = 0, v = 0, ur = 0, vc = 0;
        int lvl = 0;
        bool cand = row >= 0;
        if (cand) {   // mnLastFrameSeen == mCurrentFrame.mnId (:1328)
            unsigned h = ((unsigned)row * 2654435761u) >> 18;
            for (;;) {
                const int v0 = hs[h];
                if (v0 == -1) break;
                if (v0 == row) {
                    cand = false;
                    break;
                }
                h = (h + 1) & (HS - 1);
            }
        }
        if (cand) {
            hobs = M.has_obs[row];
            const float pw[3] = {M.pos[3 * (size_t)row], M.pos[3 * (size_t)row + 1], M.pos[3 * (size_t)row + 2]};
            float pc[3];
            xform3(R, t, pw, pc);
            if (!(pc[2] < 0.0f)) {
                const float invz = __fdiv_rn(1.0f, pc[2]);
                const float uu = __fadd_rn(__fmul_rn(__fmul_rn(S.fx, pc[0]), invz), S.cx);
                const float vv = __fadd_rn(__fmul_rn(__fmul_rn(S.fy, pc[1]), invz), S.cy);
                if (!(uu < S.min_x || uu > S.max_x) && !(vv < S.min_y || vv > S.max_y)) {
                    const float PO[3] = {__fsub_rn(pw[0], Ow[0]), __fsub_rn(pw[1], Ow[1]), __fsub_rn(pw[2], Ow[2])};
                    const float dist = norm3d(PO);
                    // the range gate uses Get{Min,Max}DistanceInvariance() = 0.8f * mfMinDistance / 1.2f * mfMaxDistance
                    // (src/MapPoint.cc:413-423), PredictScale the raw mfMaxDistance (:427-459): the table carries the raw members
                    const float maxd = M.max_dist[row], mind = M.min_dist[row];
                    if (!(dist < __fmul_rn(0.8f, mind) || dist > __fmul_rn(1.2f, maxd))) {
                        const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)M.normal[3 * (size_t)row]),
                                                               __dmul_rn((double)PO[1], (double)M.normal[3 * (size_t)row + 1])),
                                                     __dmul_rn((double)PO[2], (double)M.normal[3 * (size_t)row + 2]));
                        const float viewCos = (float)__ddiv_rn(dot, (double)dist);
                        if (!(viewCos < cos_limit)) {
                            const float ratio = __fdiv_rn(maxd, dist);
                            const float lg = (float)log((double)ratio);
                            int nScale = (int)ceilf(__fdiv_rn(lg, S.log_scale_factor));
                            if (nScale < 0) nScale = 0;
                            else if (nScale >= S.n_levels) nScale = S.n_levels - 1;
                            ok = 1;
                            u = uu;
                            v = vv;
                            ur = __fsub_rn(uu, __fmul_rn(S.mbf, invz));
                            lvl = nScale;
                            vc = viewCos;
                        }
                    }
                }
            }
        }
        L.in_view[lo + q] = ok;
        L.has_obs[lo + q] = hobs;
        L.proj_x[lo + q] = u;
        L.proj_y[lo + q] = v;
        L.proj_xr[lo + q] = ur;
        L.pred_level[lo + q] = lvl;
        L.view_cos[lo + q] = vc;
        L.desc_idx[lo + q] = row < 0 ? 0 : row;
    }
}

__device__ __forceinline__ ProjMpDev local_of(const LocalDev &L, const MapPointsDev &M, int b)
{
    ProjMpDev P;
    const size_t lo = (size_t)b * L.n_local;
    P.n_mp = L.n_local;
    P.track_in_view = L.in_view + lo;
    P.desc = M.desc;
    P.has_obs = L.has_obs + lo;
    P.pred_level = L.pred_level + lo;
    P.view_cos = L.view_cos + lo;
    P.proj_x = L.proj_x + lo;
    P.proj_y = L.proj_y + lo;
    P.proj_xr = L.proj_xr + lo;
    P.desc_idx = L.desc_idx + lo;
    return P;
}

__global__ __launch_bounds__(64 * kEntryWaves) void frames_local_entries_kernel(FramesDev S, MapPointsDev M, LocalDev L, float th, QuerySlot *slots,
                                                                  Entry *pool, int32_t *overflow, int phase, QueryRec *rec)
{
    const int b = blockIdx.y, q = kEntryWaves * blockIdx.x + (threadIdx.x >> 6);
    if (q >= L.n_local) return;
    const FrameDev F = frame_of(S, b);
    const ProjMpDev P = local_of(L, M, b);
    proj_mp_entries_body(F, P, th, slots + (size_t)b * L.n_local, pool, overflow, 0, q, 0, phase, rec + (size_t)b * L.n_local);
}

__global__ __launch_bounds__(256) void frames_local_count_kernel(FramesDev S, MapPointsDev M, LocalDev L, float th, QuerySlot *slots,
                                                                QueryRec *rec)
{
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    if (q >= L.n_local) return;
    const FrameDev F = frame_of(S, b);
    const ProjMpDev P = local_of(L, M, b);
    proj_mp_entries_body<true>(F, P, th, slots + (size_t)b * L.n_local, nullptr, nullptr, 0, q, 0, 1, rec + (size_t)b * L.n_local);
}

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void frames_local_resolve_kernel(FramesDev S, MapPointsDev M, LocalDev L, float nnratio,
                                                                   const QuerySlot *__restrict__ slots, const Entry *__restrict__ pool,
                                                                   int32_t *match_f, int32_t *nmatches, int32_t *choice,
                                                                   int32_t *nmatches_user)
{
    const int b = blockIdx.x;
    const FrameDev F = frame_of(S, b);
    const ProjMpDev P = local_of(L, M, b);
    proj_mp_resolve_fix_body<512>(F, P, nnratio, slots + (size_t)b * L.n_local, pool, match_f + (size_t)b * S.cap, nmatches + b,
                                  choice + (size_t)b * L.n_local);
    __syncthreads();
    // F.mvpMapPoints[bestIdx] = pMP (:94) -- same launch
    for (int j = threadIdx.x; j < S.n[b]; j += 512) {
        const size_t o = (size_t)b * S.cap + j;
        const int m = match_f[o];
        if (m >= 0) {
            const size_t lo = (size_t)b * L.n_local + m;
            S.mp[o] = L.local[lo];
            S.mp_state[o] = L.has_obs[lo] ? 2 : 1;
        }
    }
    if (threadIdx.x == 0 && nmatches_user) nmatches_user[b] = nmatches[b];
}

__global__ void frames_set_state_kernel(FramesDev S, MapPointsDev M)
{
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.cap) return;
    const size_t o = (size_t)b * S.cap + i;
    const int row = S.mp[o];
    S.mp_state[o] = (i < S.n[b] && row >= 0) ? (M.has_obs[row] ? 2 : 1) : 0;
}

int frames_init(aos2_frames *f)
{
    int st = bind_device(f->device);
    if (st) return st;
    if (f->dev_ready) return AOS2_OK;
    if (int st_ = stream_create(&f->stream, false)) return st_;
    // member arrays
    FramesDev &D = f->D;
    const size_t B = (size_t)D.batch, n = B * (size_t)D.cap;
    Regions<13> R;
    R.add(D.kp_x, n); R.add(D.kp_y, n); R.add(D.kp_angle, n); R.add(D.kp_octave, n); R.add(D.u_right, n); R.add(D.depth, n);
    R.add(D.grid_off, B * (kFrGridCells + 1)); R.add(D.grid_idx, n); R.add(D.mp, n); R.add(D.mp_seen, n);
    R.add(D.mp_state, n); R.add(D.outlier, n); R.add(D.Tcw, 16 * B);
    if ((st = f->mem.alloc(R.bytes() + 256))) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(f->mem.p, 0, R.bytes(), f->stream));
    R.bind(f->mem.p);
    // the sticky overflow word lives in page-locked HOST memory the kernels write through (rarely: only when a frame's windows did
    // not fit): aos2_frames_wait reads it after the stream has drained, without a copy -- a 4-byte device-to-host copy behind the
    // last kernel cost ~35 us of a single frame's 0.68 ms
    if ((st = f->h_overflow.alloc(16))) return st;
    memset(f->h_overflow.p, 0, 16 * sizeof(int32_t));
    f->d_overflow = f->h_overflow.p;
    if ((st = f->tables.alloc(64))) return st;
    if ((st = f->h_tables.alloc(16))) return st;
    f->dev_ready = true;
    return AOS2_OK;
}

// scratch of the two searches: per-frame query slots, decisions, per-feature results
struct FrScratch {
    QuerySlot *slots;
    QueryRec *rec;
    int32_t *choice, *match_f, *nmatches;
    uint32_t *bin_f;
    LocalDev L;
    Entry *pool;
    int share;
};

// The two searches lay the one `scratch` buffer out differently (their query and local-point counts differ): each runs to
// its end on the batch's stream before the next one starts there, so neither sees the other's layout.
static int frames_scratch(aos2_frames *f, int nq_cap, int n_local, FrScratch &X)
{
    const size_t B = (size_t)f->D.batch, nf = B * (size_t)f->D.cap;
    const size_t nq = B * (size_t)nq_cap, nl = B * (size_t)n_local;
    LocalDev &L = X.L;
    Regions<14> R;
    R.add(X.slots, nq); R.add(X.choice, nq); R.add(X.match_f, nf); R.add(X.bin_f, nf); R.add(X.nmatches, B); R.add(X.rec, nq);
    R.add(L.in_view, nl); R.add(L.has_obs, nl); R.add(L.proj_x, nl); R.add(L.proj_y, nl); R.add(L.proj_xr, nl); R.add(L.view_cos, nl);
    R.add(L.pred_level, nl); R.add(L.desc_idx, nl);
    int st;
    if ((st = f->scratch.alloc(R.bytes() + 256))) return st;
    R.bind(f->scratch.p);
    L.n_local = n_local; L.local = nullptr;
    // entry pool: `share` entries per frame = its queries x the average window population budgeted (the windows of
    // a frame share it; AOS2_FRAMES_WINDOW_BUDGET, default 64 features per window on average)
    int budget = 64;
    if (const char *v = getenv("AOS2_FRAMES_WINDOW_BUDGET")) budget = std::max(1, atoi(v));
    const size_t share = (size_t)nq_cap * (size_t)budget;
    if (share * B > ((size_t)1 << 31) - 1) {
        set_error("frame batch of %zu x %d queries exceeds the entry pool's index range", B, nq_cap);
        return AOS2_ERR_ARG;
    }
    if ((st = f->pool.alloc(share * B + 1))) return st;
    X.pool = reinterpret_cast<Entry *>(f->pool.p);
    X.share = (int)share;
    return AOS2_OK;
}

// One Frame member array as include/aos2.h documents it (AOS2_FRAMES_*): where it lies, its element size, its elements per
// frame, and whether aos2_frames_get copies it out (the others are "device pointer only").  An unknown id has no array.
struct FrameMember {
    const void *p;
    size_t elem, per_frame;
    bool gettable;
};

template <class T>
static FrameMember member_of(const T *p, size_t per_frame, bool gettable) { return FrameMember{p, sizeof(T), per_frame, gettable}; }

static FrameMember frame_member(const FramesDev &D, int what)
{
    const size_t cap = (size_t)D.cap;
    switch (what) {
    case AOS2_FRAMES_MAP_POINTS: return member_of(D.mp, cap, true);
    case AOS2_FRAMES_OUTLIER: return member_of(D.outlier, cap, true);
    case AOS2_FRAMES_TCW: return member_of(D.Tcw, 16, true);
    case AOS2_FRAMES_U_RIGHT: return member_of(D.u_right, cap, true);
    case AOS2_FRAMES_DEPTH: return member_of(D.depth, cap, true);
    case AOS2_FRAMES_GRID_OFF: return member_of(D.grid_off, kFrGridCells + 1, true);
    case AOS2_FRAMES_GRID_IDX: return member_of(D.grid_idx, cap, true);
    case AOS2_FRAMES_KEYS_UN_X: return member_of(D.kp_x, cap, true);
    case AOS2_FRAMES_KEYS_UN_Y: return member_of(D.kp_y, cap, true);
    case AOS2_FRAMES_KEYS_ANGLE: return member_of(D.kp_angle, cap, false);
    case AOS2_FRAMES_KEYS_OCTAVE: return member_of(D.kp_octave, cap, false);
    default: return FrameMember{nullptr, 0, 0, false};
    }
}

}  // namespace aos2

using namespace aos2;

extern "C" {

int aos2_frames_create(int device, int batch, int cap, aos2_frames_t **out)
{
    if (!out || batch <= 0 || cap <= 0 || cap > 5632) {   // (the parallel greedy resolve keeps 8 B per feature in LDS)
        set_error("bad frame batch (batch %d, cap %d)", batch, cap);
        return AOS2_ERR_ARG;
    }
    aos2_frames *f = new aos2_frames();
    f->device = device;
    f->D.batch = batch;
    f->D.cap = cap;
    *out = f;
    return AOS2_OK;
}

void aos2_frames_destroy(aos2_frames_t *f)
{
    if (!f) return;
    if (f->dev_ready) {
        (void)hipSetDevice(f->device);
        (void)hipStreamSynchronize(f->stream);
        f->mem.release(); f->tables.release(); f->scratch.release(); f->pool.release(); f->pose_mem.release();
        f->h_tables.release(); f->h_overflow.release();
        for (KfStage &k : f->kf) {
            k.host.release(); k.dev.release();
            if (k.uploaded) (void)hipEventDestroy(k.uploaded);
        }
        if (f->order_ev) (void)hipEventDestroy(f->order_ev);
        if (f->ext_ev) (void)hipEventDestroy(f->ext_ev);
        (void)hipStreamDestroy(f->stream);
    }
    delete f;
}

void *aos2_frames_stream(aos2_frames_t *f)
{
    if (!f || frames_init(f)) return nullptr;
    return f->stream;
}

const void *aos2_frames_device_ptr(aos2_frames_t *f, int what)
{
    if (!f || !f->dev_ready) return nullptr;
    return frame_member(f->D, what).p;
}

int aos2_frames_wait(aos2_frames_t *f)
{
    if (!f) return AOS2_ERR_ARG;
    if (!f->dev_ready) return AOS2_OK;
    int st = bind_device(f->device);
    if (st) return st;
    {   // (a host wait inside aos2_capture_begin / _end would invalidate the recording: refused before the runtime sees it)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(f->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            set_error("aos2_frames_wait: the batch's stream is recording (aos2_capture_begin); a host wait cannot be recorded");
            return AOS2_ERR_ARG;
        }
    }
    AOS2_HIP_CHECK(hipStreamSynchronize(f->stream));
    AOS2_HIP_CHECK(hipGetLastError());
    volatile int32_t *h = f->h_overflow.p;
    if (h[0] > 0) {
        const int need = h[0];
        h[0] = 0;   // (nothing is in flight on the batch's stream)
        set_error("frame batch: the search windows of one frame held %d features, more than the frame's share of the entry "
                  "pool (raise AOS2_FRAMES_WINDOW_BUDGET); that frame found no matches", need);
        return AOS2_ERR_CAPACITY;
    }
    return AOS2_OK;
}

static int frames_build_any(aos2_frames_t *f, aos2_extractor_t *e, int batch, const aos2_keypoint_t *d_kps, const uint8_t *d_desc,
                            const int32_t *d_n, int cap, int w, int h, const float *d_depth, int depth_stride,
                            size_t depth_image_stride, const float *d_u_right, const float *d_depth_kp, float fx, float fy, float cx,
                            float cy, float mbf)
{
    if (!f || !e || !d_kps || !d_desc || !d_n || batch != f->D.batch || cap != f->D.cap || w <= 0 || h <= 0 ||
        (d_depth && depth_stride < w)) {
        set_error("bad argument (the batch and keypoint capacity are those of aos2_frames_create)");
        return AOS2_ERR_ARG;
    }
    int st = frames_init(f);
    if (st) return st;
    FramesDev &D = f->D;
    const int L = aos2_extractor_levels(e);
    if (L <= 0 || L > 8) {
        set_error("unsupported number of pyramid levels %d", L);
        return AOS2_ERR_ARG;
    }
    // mvScaleFactors, mvInvLevelSigma2 (Frame.cc:94-100 copies them from the extractor)
    float *ht = f->h_tables.p;   // [0, 8) scale factors, [8, 16) inverse level sigma2
    memcpy(ht, aos2_extractor_scale_factors(e), sizeof(float) * L);
    memcpy(ht + 8, aos2_extractor_inv_sigma2(e), sizeof(float) * L);
    AOS2_HIP_CHECK(hipMemcpyAsync(f->tables.p, ht, sizeof(float) * 16, hipMemcpyHostToDevice, f->stream));
    D.n_levels = L;
    D.scale_factors = f->tables.p;
    D.inv_level_sigma2 = f->tables.p + 8;
    D.n = d_n; D.kps = d_kps; D.desc = d_desc;
    // Frame::ComputeImageBounds (:463-493): the image, or its four corners undistorted
    D.has_dist = f->dist[0] != 0.0f ? 1 : 0;
    memcpy(D.dist, f->dist, sizeof(D.dist));
    {
        float bd[4];
        aos2_frame_image_bounds(w, h, fx, fy, cx, cy, f->dist, bd);
        D.min_x = bd[0]; D.max_x = bd[1]; D.min_y = bd[2]; D.max_y = bd[3];
    }
    D.grid_w_inv = (float)kFrGridCols / (D.max_x - D.min_x);   // static_cast<float>(FRAME_GRID_COLS) / (mnMaxX - mnMinX) :154
    D.grid_h_inv = (float)kFrGridRows / (D.max_y - D.min_y);
    D.fx = fx; D.fy = fy; D.cx = cx; D.cy = cy; D.mbf = mbf;
    D.mb = mbf / fx;   // mb = mbf / fx (:163)
    D.log_scale_factor = (float)log((double)aos2_extractor_scale_factor(e));   // mfLogScaleFactor = log(mfScaleFactor) :95
    if ((st = aos2_extractor_stream_wait(e, f->stream))) return st;
    const size_t lds = (size_t)(kFrGridCells + 1) * 4 + (size_t)cap * 2 + 16;
    hipLaunchKernelGGL(frames_build_kernel, dim3(batch), dim3(256), lds, f->stream, D, d_depth, depth_stride, depth_image_stride, d_u_right,
                       d_depth_kp);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

int aos2_frames_build(aos2_frames_t *f, aos2_extractor_t *e, int batch, const aos2_keypoint_t *d_kps, const uint8_t *d_desc,
                      const int32_t *d_n, int cap, int w, int h, const float *d_depth, int depth_stride,
                      size_t depth_image_stride, float fx, float fy, float cx, float cy, float mbf)
{
    return frames_build_any(f, e, batch, d_kps, d_desc, d_n, cap, w, h, d_depth, depth_stride, depth_image_stride, nullptr, nullptr, fx, fy,
                            cx, cy, mbf);
}

int aos2_frames_build_stereo(aos2_frames_t *f, aos2_extractor_t *e_left, int batch, const aos2_keypoint_t *d_kps, const uint8_t *d_desc,
                             const int32_t *d_n, int cap, int w, int h, const float *d_u_right, const float *d_depth_kp, float fx,
                             float fy, float cx, float cy, float mbf)
{
    if (!d_u_right || !d_depth_kp) {
        set_error("bad argument (mvuRight / mvDepth of ComputeStereoMatches)");
        return AOS2_ERR_ARG;
    }
    return frames_build_any(f, e_left, batch, d_kps, d_desc, d_n, cap, w, h, nullptr, w, (size_t)w * h, d_u_right, d_depth_kp, fx, fy, cx,
                            cy, mbf);
}

// Frame::ComputeImageBounds (src/Frame.cc:463-493): once per camera, four points, on the host
int aos2_frame_image_bounds(int w, int h, float fx, float fy, float cx, float cy, const float *dist5, float *bounds4)
{
    if (!dist5 || !bounds4 || w <= 0 || h <= 0) return AOS2_ERR_ARG;
    bounds4[0] = 0.f; bounds4[1] = (float)w; bounds4[2] = 0.f; bounds4[3] = (float)h;   // mnMinX mnMaxX mnMinY mnMaxY
    if (dist5[0] != 0.0f) {
        float c[4][2];
        const float corner[4][2] = {{0.f, 0.f}, {(float)w, 0.f}, {0.f, (float)h}, {(float)w, (float)h}};
        for (int i = 0; i < 4; ++i) undistort_point(fx, fy, cx, cy, dist5, corner[i][0], corner[i][1], c[i][0], c[i][1]);
        bounds4[0] = std::min(c[0][0], c[2][0]);
        bounds4[1] = std::max(c[1][0], c[3][0]);
        bounds4[2] = std::min(c[0][1], c[1][1]);
        bounds4[3] = std::max(c[2][1], c[3][1]);
    }
    return AOS2_OK;
}

int aos2_frames_set_distortion(aos2_frames_t *f, float k1, float k2, float p1, float p2, float k3)
{
    if (!f) return AOS2_ERR_ARG;
    f->dist[0] = k1; f->dist[1] = k2; f->dist[2] = p1; f->dist[3] = p2; f->dist[4] = k3;
    return AOS2_OK;
}

int aos2_frames_set_pose(aos2_frames_t *f, const float *d_Tcw)
{
    if (!f || !d_Tcw) return AOS2_ERR_ARG;
    int st = frames_init(f);
    if (st) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(f->D.Tcw, d_Tcw, 64 * (size_t)f->D.batch, hipMemcpyDeviceToDevice, f->stream));
    return AOS2_OK;
}

int aos2_frames_set_map_points(aos2_frames_t *f, const int32_t *mp, const uint8_t *outlier, const aos2_map_points_dev_t *table)
{
    if (!f || !mp || !table || !f->dev_ready || !f->D.n) {
        set_error("bad argument (aos2_frames_build comes first)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(f->device);
    if (st) return st;
    const size_t n = (size_t)f->D.batch * f->D.cap;
    AOS2_HIP_CHECK(hipMemcpyAsync(f->D.mp, mp, 4 * n, hipMemcpyHostToDevice, f->stream));
    if (outlier) AOS2_HIP_CHECK(hipMemcpyAsync(f->D.outlier, outlier, n, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(frames_set_state_kernel, dim3((f->D.cap + 255) / 256, f->D.batch), dim3(256), 0, f->stream, f->D,
                       map_points_dev(table));
    AOS2_HIP_CHECK(hipStreamSynchronize(f->stream));   // (the host array may be released by the caller)
    return AOS2_OK;
}

int aos2_frames_get(aos2_frames_t *f, int what, void *dst, size_t bytes)
{
    if (!f || !dst || !f->dev_ready) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(f->device);
    if (st) return st;
    const FrameMember m = frame_member(f->D, what);
    if (!m.gettable) {
        set_error("unknown member %d", what);
        return AOS2_ERR_ARG;
    }
    const size_t have = m.elem * m.per_frame * (size_t)f->D.batch;
    if (bytes != have) {
        set_error("member %d holds %zu bytes, %zu requested", what, have, bytes);
        return AOS2_ERR_ARG;
    }
    AOS2_HIP_CHECK(hipMemcpyAsync(dst, m.p, have, hipMemcpyDeviceToHost, f->stream));
    AOS2_HIP_CHECK(hipStreamSynchronize(f->stream));
    return AOS2_OK;
}

int aos2_frames_search_by_projection_last(aos2_frames_t *cur, const aos2_frames_t *last, const aos2_map_points_dev_t *mps, float th,
                                          int mono, int check_orientation, int32_t *d_nmatches)
{
    if (!cur || !last || !mps || !cur->dev_ready || !last->dev_ready || cur->D.batch != last->D.batch || !cur->D.n || !last->D.n) {
        set_error("bad argument (both batches built, same number of frames)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(cur->device);
    if (st) return st;
    FrScratch X;
    if ((st = frames_scratch(cur, last->D.cap, 1, X))) return st;
    const FramesDev &C = cur->D, &Lf = last->D;
    const MapPointsDev M = map_points_dev(mps);
    hipStream_t q = cur->stream;
    const int B = C.batch;
    if (last != cur && (st = order_behind(q, last))) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(X.slots, 0, sizeof(QuerySlot) * (size_t)B * Lf.cap, q));
    if (B >= 8)   // a thread per query; a few frames fill the device better with a wave per query
        hipLaunchKernelGGL(frames_last_count_kernel, dim3((Lf.cap + 255) / 256, B), dim3(256), 0, q, C, Lf, M, th, mono ? 1 : 0, X.slots, X.rec);
    else
        hipLaunchKernelGGL(frames_last_entries_kernel, dim3((Lf.cap + kEntryWaves - 1) / kEntryWaves, B), dim3(64 * kEntryWaves), 0, q, C, Lf, M, th, mono ? 1 : 0, X.slots, X.pool,
                           cur->d_overflow, 1, X.rec);
    // (a one-pass variant -- every query takes its entries behind a per-frame atomic cursor -- was measured: the ~1000 same-address
    // atomics of a frame cost what the counting pass + scan cost, 0.094 vs 0.095 ms per frame, and 256 frames got slower)
    hipLaunchKernelGGL(frames_scan_slots_kernel, dim3(B), dim3(256), 0, q, X.slots, Lf.n, Lf.cap, X.share, cur->d_overflow);
    hipLaunchKernelGGL(frames_last_entries_kernel, dim3((Lf.cap + kEntryWaves - 1) / kEntryWaves, B), dim3(64 * kEntryWaves), 0, q, C, Lf, M, th, mono ? 1 : 0, X.slots, X.pool,
                       cur->d_overflow, 2, X.rec);
    if (Lf.cap > 3 * 512)   // (kFixQpt queries per thread stay in registers)
        hipLaunchKernelGGL(frames_last_resolve_kernel<1024>, dim3(B), dim3(1024), (size_t)C.cap * 8 + 16, q, C, Lf, M, check_orientation ? 1 : 0,
                           X.slots, X.pool, X.match_f, X.bin_f, X.nmatches, X.choice, d_nmatches);
    else
        hipLaunchKernelGGL(frames_last_resolve_kernel<512>, dim3(B), dim3(512), (size_t)C.cap * 8 + 16, q, C, Lf, M, check_orientation ? 1 : 0,
                           X.slots, X.pool, X.match_f, X.bin_f, X.nmatches, X.choice, d_nmatches);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

int aos2_frames_wait_for_stream(aos2_frames_t *f, void *hip_stream)
{
    if (!f) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = frames_init(f);
    if (st) return st;
    hipStream_t producer = static_cast<hipStream_t>(hip_stream);
    // (a stream wait captures the event's state at the time of the call, so the one event serves several producers back to back)
    if (!f->ext_ev) AOS2_HIP_CHECK(hipEventCreateWithFlags(&f->ext_ev, hipEventDisableTiming));
    AOS2_HIP_CHECK(hipEventRecord(f->ext_ev, producer));
    AOS2_HIP_CHECK(hipStreamWaitEvent(f->stream, f->ext_ev, 0));
    return AOS2_OK;
}

int aos2_frames_discard_outliers(aos2_frames_t *f)
{
    if (!f || !f->dev_ready || !f->D.n) return AOS2_ERR_ARG;
    int st = bind_device(f->device);
    if (st) return st;
    hipLaunchKernelGGL(frames_discard_kernel, dim3((f->D.cap + 255) / 256, f->D.batch), dim3(256), 0, f->stream, f->D);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

int aos2_frames_search_local_points(aos2_frames_t *f, const aos2_map_points_dev_t *mps, const int32_t *d_local, int n_local, float th,
                                    float nnratio, int32_t *d_nmatches)
{
    if (!f || !mps || !d_local || n_local <= 0 || !f->dev_ready || !f->D.n || !mps->normal || !mps->min_dist || !mps->max_dist ||
        f->D.cap > 4096) {
        set_error("bad argument (local map points need normals and distance ranges; at most 4096 features per frame)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(f->device);
    if (st) return st;
    FrScratch X;
    if ((st = frames_scratch(f, n_local, n_local, X))) return st;
    X.L.local = d_local;
    const FramesDev &S = f->D;
    const MapPointsDev M = map_points_dev(mps);
    hipStream_t q = f->stream;
    const int B = S.batch;
    hipLaunchKernelGGL(frames_frustum_kernel, dim3(B), dim3(256), 0, q, S, M, X.L, 0.5f);
    if (B >= 8)
        hipLaunchKernelGGL(frames_local_count_kernel, dim3((n_local + 255) / 256, B), dim3(256), 0, q, S, M, X.L, th, X.slots, X.rec);
    else
        hipLaunchKernelGGL(frames_local_entries_kernel, dim3((n_local + kEntryWaves - 1) / kEntryWaves, B), dim3(64 * kEntryWaves), 0, q, S, M, X.L, th, X.slots, X.pool, f->d_overflow, 1, X.rec);
    hipLaunchKernelGGL(frames_scan_slots_kernel, dim3(B), dim3(256), 0, q, X.slots, (const int32_t *)nullptr, n_local, X.share,
                       f->d_overflow);
    hipLaunchKernelGGL(frames_local_entries_kernel, dim3((n_local + kEntryWaves - 1) / kEntryWaves, B), dim3(64 * kEntryWaves), 0, q, S, M, X.L, th, X.slots, X.pool, f->d_overflow, 2, X.rec);
    hipLaunchKernelGGL(frames_local_resolve_kernel, dim3(B), dim3(512), (size_t)S.cap * 8 + 16, q, S, M, X.L, nnratio, X.slots, X.pool,
                       X.match_f, X.nmatches, X.choice, d_nmatches);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

}  // extern "C"
