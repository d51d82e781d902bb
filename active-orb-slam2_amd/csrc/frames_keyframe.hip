// Keyframe work on device-resident frame batches (include/aos2.h): SearchForTriangulation, the search part of Fuse, and the loop
// body of LocalMapping::CreateNewMapPoints for the matches the first left in HBM.  A keyframe is a frame of a built batch
// (frames.hip).  The searches use the device routines of search_device.h; the triangulation arithmetic is csrc/triangulate.h,
// shared with the host-pointer form (triangulate.hip) and the host tap.
#include <algorithm>
#include <vector>

#include "frames.h"
#include "search_device.h"
#include "triangulate.h"

namespace aos2 {

// ---------------------------------------------------------------------------------------------------------------
// Keyframe work on device-resident batches (LocalMapping::CreateNewMapPoints / SearchInNeighbors, src/LocalMapping.cc:272, 493):
// a keyframe is a frame of a built batch -- KeyFrame::KeyFrame copies exactly these Frame members (src/KeyFrame.cc:37-62).
// ---------------------------------------------------------------------------------------------------------------
struct FrTriPair {
    int32_t kf1, kf2;
    float F12[9], ex, ey;
};

// SearchForTriangulation (src/ORBmatcher.cc:657-823) for pairs (frame kf1 of A, frame kf2 of B): one wave per KF1 feature.
// vbMatched2 is never set by the reference, so the KF1 features are independent (triang_match_kernel above): a feature
// without a map point looks its vocabulary node (node_of, the FeatureVector key of the feature) up in KF2's FeatureVector
// (binary search over <= a few hundred ascending node ids) and takes the best candidate of that bucket.  The reference walks
// KF1's FeatureVector (:688-700), which holds a feature only if its word has a non-zero weight (DBoW2 transform): the feature
// has to be in its node's bucket of KF1's FeatureVector too.
struct FrFvDev {
    const int32_t *node, *off, *idx, *n;
};

// position of `node` in the ascending id list of a FeatureVector, -1 if absent (one thread: ~7 dependent loads of a hot list)
__device__ __forceinline__ int fv_find_node(const int32_t *ids, int nn, int node)
{
    int lo = 0, hi = nn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < node) lo = mid + 1; else hi = mid;
    }
    return (lo < nn && ids[lo] == node) ? lo : -1;
}

// SearchForTriangulation's matching loop (src/ORBmatcher.cc:690-773) for a list of keyframe pairs: one THREAD per feature of
// KF1 (round 3: one wave per feature -- 655 k one-wave workgroups per 640 pairs whose lanes mostly idled: a vocabulary node at
// levelsup 4 holds ~10 features of a keyframe).  The thread walks the bucket of KF2 in its order and keeps the LAST smallest
// distance (`dist > bestDist` continues, :734: a tie replaces).  vbMatched2 is never set by the reference, so the features
// are independent.
__global__ __launch_bounds__(256) void frames_triang_match_kernel(FramesDev A, FramesDev B, const FrTriPair *__restrict__ pairs,
                                                                 const uint32_t *__restrict__ node_of1, FrFvDev fv1, const int32_t *__restrict__ fv_node2,
                                                                 const int32_t *__restrict__ fv_off2, const int32_t *__restrict__ fv_idx2,
                                                                 const int32_t *__restrict__ n_fv2, int only_stereo, int32_t *__restrict__ match12)
{
    const FrTriPair &P = pairs[blockIdx.y];
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    if (i1 >= A.cap) return;
    const size_t o1 = (size_t)P.kf1 * A.cap, o2 = (size_t)P.kf2 * B.cap;
    int32_t *out = match12 + (size_t)blockIdx.y * A.cap;
    int best = -1;   // vMatches12(pKF1->N, -1) :681
    do {
        if (i1 >= A.n[P.kf1]) break;
        if (A.mp[o1 + i1] >= 0) break;                                // pKF1->GetMapPoint(idx1) :700-703
        const bool bStereo1 = A.u_right[o1 + i1] >= 0;
        if (only_stereo && !bStereo1) break;                          // :705-709
        // the bucket of KF2 with this feature's node id
        const int node = (int)node_of1[o1 + i1];
        const int lo = fv_find_node(fv_node2 + o2, n_fv2[P.kf2], node);
        if (lo < 0) break;
        {
            const int l1 = fv_find_node(fv1.node + o1, fv1.n[P.kf1], node);
            if (l1 < 0) break;
            const int32_t *off1 = fv1.off + (size_t)P.kf1 * (A.cap + 1);
            const int beg = off1[l1], cnt = off1[l1 + 1] - beg;
            const int32_t *b1 = fv1.idx + o1 + beg;
            bool mine = false;
            for (int j = 0; j < cnt && !mine; ++j) mine = b1[j] == i1;
            if (!mine) break;
        }
        const int32_t *off2 = fv_off2 + (size_t)P.kf2 * (B.cap + 1);
        const int f_beg = off2[lo], f_cnt = off2[lo + 1] - f_beg;
        const int32_t *bucket = fv_idx2 + o2 + f_beg;
        const Desc d1 = load_desc(A.desc + (o1 + i1) * 32);
        const float kx = A.kp_x[o1 + i1], ky = A.kp_y[o1 + i1];
        const EpiLine line = epi_line(P.F12, kx, ky);
        int bestDist = TH_LOW;
        for (int j = 0; j < f_cnt; ++j) {
            const int idx2 = bucket[j];
            if (B.mp[o2 + idx2] >= 0) continue;                       // :723
            const bool bStereo2 = B.u_right[o2 + idx2] >= 0;
            if (only_stereo && !bStereo2) continue;
            const int dist = hamming(d1, load_desc(B.desc + (o2 + idx2) * 32));
            if (dist > TH_LOW || dist > bestDist) continue;           // :734
            const float sf = B.scale_factors[B.kp_octave[o2 + idx2]];
            // mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i] (ORBextractor.cc:420)
            if (!epi_admits(line, B.kp_x[o2 + idx2], B.kp_y[o2 + idx2], !bStereo1 && !bStereo2, P.ex, P.ey, sf, __fmul_rn(sf, sf)))
                continue;
            best = idx2;
            bestDist = dist;
        }
    } while (false);
    out[i1] = best;
}

// rotation consistency (:776-808) + count, one wave per pair
__global__ __launch_bounds__(64) void frames_triang_finish_kernel(FramesDev A, FramesDev B, const FrTriPair *__restrict__ pairs, int check_ori,
                                                                  int32_t *__restrict__ match12, int32_t *__restrict__ nmatches)
{
    const FrTriPair &P = pairs[blockIdx.x];
    triang_finish_body(A.n[P.kf1], A.kp_angle + (size_t)P.kf1 * A.cap, B.kp_angle + (size_t)P.kf2 * B.cap,
                       match12 + (size_t)blockIdx.x * A.cap, nmatches + blockIdx.x, check_ori);
}

__device__ const uint8_t k_valid_one = 1;

// the search part of Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:825-975) for problems (target keyframe = a frame of the
// batch, candidate map points = rows of the table, -1 = the loop head rejected it).  One THREAD per candidate: the window of a
// fused point holds a handful of features (radius th x scale: 3-4 grid columns of a sparse grid), so a wave per candidate
// (round 3's form: 2 M one-wave workgroups per step, 1.66 ms) left ~60 lanes idle in the window loop and repeated the setup
// in every lane.  The thread visits the window in GetFeaturesInArea's order (columns, cells of a column, the features of a
// cell in their CSR order) and keeps the FIRST smallest distance -- `if (dist < bestDist)` of :937-941.
__global__ __launch_bounds__(256) void frames_fuse_kernel(FramesDev S, MapPointsDev M, const int32_t *__restrict__ target,
                                                         const int32_t *__restrict__ rows, int n_pts, float th,
                                                         int32_t *__restrict__ best_idx, int32_t *__restrict__ best_dist)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, b = target[p];
    if (i >= n_pts) return;
    const size_t o = (size_t)p * n_pts + i;
    const int row = rows[o];
    int bi = -1, bd = 256;
    if (row >= 0) {
        const FrameDev F = frame_of(S, b);
        const float *T = S.Tcw + (size_t)b * 16;
        ProjGenDev P;
        P.n_pts = 1; P.mode = 0;
        P.valid = &k_valid_one;
        P.desc = M.desc + (size_t)row * 32;
        P.pos = M.pos + 3 * (size_t)row; P.max_dist = M.max_dist + row; P.min_dist = M.min_dist + row; P.normal = M.normal + 3 * (size_t)row;
        P.q_angle = nullptr;
        P.inv_level_sigma2 = S.inv_level_sigma2;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) P.R[3 * r + c] = T[4 * r + c];
            P.t[r] = T[4 * r + 3];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // Ow = -Rcw.t() * tcw (KeyFrame::SetPose, src/KeyFrame.cc:64-82; cv::gemm: double accumulation)
            const double sacc = __dadd_rn(__dadd_rn(__dmul_rn((double)T[k], (double)T[3]), __dmul_rn((double)T[4 + k], (double)T[7])),
                                          __dmul_rn((double)T[8 + k], (double)T[11]));
            P.Ow[k] = (float)__dmul_rn(sacc, -1.0);
        }
        P.fx = S.fx; P.fy = S.fy; P.cx = S.cx; P.cy = S.cy; P.bf = S.mbf; P.log_scale_factor = S.log_scale_factor; P.th = th;
        const ProjSetup Q = proj_gen_setup(F, P, 0);
        if (Q.ok) {
            const Window w = window_cells(F, Q.u, Q.v, Q.radius);
            if (w.ok) {
                const Desc dq = load_desc(P.desc);
                int best = 256, arg = -1;
                for (int ix = w.x0; ix <= w.x1; ++ix) {
                    const int j0 = F.grid_off[ix * GRID_ROWS + w.y0], j1 = F.grid_off[ix * GRID_ROWS + w.y1 + 1];   // (a column's cells are neighbours in the CSR)
                    for (int j = j0; j < j1; ++j) {
                        const int idx = F.grid_idx[j];
                        const float kx = F.kp_x[idx], ky = F.kp_y[idx];
                        const int oct = F.kp_octave[idx];
                        const float kr = F.u_right[idx];
                        if (!(fabsf(__fsub_rn(kx, Q.u)) < Q.radius && fabsf(__fsub_rn(ky, Q.v)) < Q.radius)) continue;
                        if (oct < Q.level - 1 || oct > Q.level) continue;
                        // reprojection error gates of Fuse (:911-935)
                        const float ex = __fsub_rn(Q.u, kx), ey = __fsub_rn(Q.v, ky);
                        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                        double lim = 5.99;
                        if (kr >= 0) {
                            const float er = __fsub_rn(Q.ur, kr);
                            e2 = __fadd_rn(e2, __fmul_rn(er, er));
                            lim = 7.8;
                        }
                        if ((double)__fmul_rn(e2, P.inv_level_sigma2[oct]) > lim) continue;
                        const int dist = hamming(dq, load_desc(F.desc_f + (size_t)idx * 32));
                        if (dist < best) {
                            best = dist;
                            arg = idx;
                        }
                    }
                }
                if (arg >= 0 && best <= TH_LOW) {
                    bi = arg;
                    bd = best;
                }
            }
        }
    }
    best_idx[o] = bi;
    best_dist[o] = bd;
}

__device__ __forceinline__ TriKf tri_kf_of(const FramesDev &S, int b)
{
    TriKf K;
    K.T = S.Tcw + (size_t)b * 16;
    K.fx = S.fx; K.fy = S.fy; K.cx = S.cx; K.cy = S.cy; K.mb = S.mb; K.mbf = S.mbf;
    K.sf = S.scale_factors;
    return K;
}

__device__ __forceinline__ TriObs tri_obs_of(const FramesDev &S, size_t o)
{
    TriObs q;
    q.ux = S.kp_x[o]; q.uy = S.kp_y[o];
    q.kx = S.kps[o].x; q.ky = S.kps[o].y;
    q.ur = S.u_right[o]; q.depth = S.depth[o];
    q.octave = S.kp_octave[o];
    return q;
}

// grid (ceil(cap of A / 256), n_pairs): thread = feature i1 of keyframe kf1[pair]
__global__ __launch_bounds__(256) void frames_triangulate_kernel(FramesDev A, FramesDev B, const int32_t *__restrict__ kf1,
                                                                const int32_t *__restrict__ kf2, const int32_t *__restrict__ match12,
                                                                float *__restrict__ x3D_out, uint8_t *__restrict__ status_out)
{
    const int p = blockIdx.y, b1 = kf1[p], b2 = kf2[p];
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    const size_t o1 = (size_t)b1 * A.cap, o2 = (size_t)b2 * B.cap, row = (size_t)p * A.cap;
    const TriKf K1 = tri_kf_of(A, b1), K2 = tri_kf_of(B, b2);
    TriObs q1 = {}, q2 = {};
    bool matched = false;
    if (i1 < A.cap && i1 < A.n[b1]) {
        const int i2 = match12[row + i1];
        if (i2 >= 0 && i2 < B.n[b2] && i2 < B.cap) {
            matched = true;
            q1 = tri_obs_of(A, o1 + i1);
            q2 = tri_obs_of(B, o2 + i2);
        }
    }
    float x3D[3];
    const int st = tri_block(matched, K1, K2, q1, q2, x3D);
    if (i1 < A.cap) {
        status_out[row + i1] = (uint8_t)st;
        float *o = x3D_out + 3 * (row + i1);
        o[0] = x3D[0]; o[1] = x3D[1]; o[2] = x3D[2];
    }
}

// The pairs of a group share keyframe 1 and stand in neighbour order: per feature the first accepted pair keeps it, later accepted
// ones are superseded (the reference's next SearchForTriangulation would have skipped the feature, src/ORBmatcher.cc:700-703).
// Without first_wins every pair is a group of its own and only the counting is left.  grid (ceil(cap / 256), n_groups).
__global__ __launch_bounds__(256) void frames_triangulate_resolve_kernel(int cap, const int32_t *__restrict__ grp_off, const int32_t *__restrict__ grp_pair,
                                                                        uint8_t *__restrict__ status, int32_t *__restrict__ nnew)
{
    const int g = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int beg = grp_off[g], end = grp_off[g + 1];
    bool taken = false;
    for (int q = beg; q < end; ++q) {
        const int p = grp_pair[q];
        const size_t o = (size_t)p * cap + i;
        bool accepted = false;
        if (i < cap && status[o] == AOS2_TRI_ACCEPTED) {
            if (taken) status[o] = AOS2_TRI_SUPERSEDED;
            else accepted = taken = true;
        }
        const int cnt = __popcll(__ballot(accepted));
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&nnew[p], cnt);
    }
}

}  // namespace aos2

using namespace aos2;

extern "C" {

int aos2_frames_search_for_triangulation(aos2_frames_t *a, aos2_frames_t *b, const aos2_frames_triang_t *q, int only_stereo,
                                         int check_orientation, int32_t *d_match12, int32_t *d_nmatches)
{
    if (!a || !b || !q || q->n_pairs <= 0 || !q->kf1 || !q->kf2 || !q->F12 || !q->epipole || !q->d_node_of1 || !q->d_fv_node1 || !q->d_fv_off1 ||
        !q->d_fv_idx1 || !q->d_n_fv1 || !q->d_fv_node2 ||
        !q->d_fv_off2 || !q->d_fv_idx2 || !q->d_n_fv2 || !d_match12 || !d_nmatches || !a->dev_ready || !b->dev_ready || !a->D.n || !b->D.n) {
        set_error("bad argument (both keyframe batches built)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(a->device);
    if (st) return st;
    const int n = q->n_pairs;
    for (int p = 0; p < n; ++p)
        if (q->kf1[p] < 0 || q->kf1[p] >= a->D.batch || q->kf2[p] < 0 || q->kf2[p] >= b->D.batch) {
            set_error("pair %d names keyframes (%d, %d) outside the batches", p, q->kf1[p], q->kf2[p]);
            return AOS2_ERR_ARG;
        }
    // the pair records
    KfStage &stage = a->kf[kKfTriang];
    FrTriPair *h;
    if ((st = kf_stage_begin(stage, (size_t)n, h))) return st;
    for (int p = 0; p < n; ++p) {
        h[p].kf1 = q->kf1[p]; h[p].kf2 = q->kf2[p];
        memcpy(h[p].F12, q->F12 + 9 * (size_t)p, 36);
        h[p].ex = q->epipole[2 * p]; h[p].ey = q->epipole[2 * p + 1];
    }
    hipStream_t s = a->stream;
    if (b != a && (st = order_behind(s, b))) return st;
    const FrTriPair *dp;
    if ((st = kf_stage_upload(a, stage, dp))) return st;
    hipLaunchKernelGGL(frames_triang_match_kernel, dim3((a->D.cap + 255) / 256, n), dim3(256), 0, s, a->D, b->D, dp, q->d_node_of1,
                       FrFvDev{q->d_fv_node1, q->d_fv_off1, q->d_fv_idx1, q->d_n_fv1}, q->d_fv_node2, q->d_fv_off2,
                       q->d_fv_idx2, q->d_n_fv2, only_stereo ? 1 : 0, d_match12);
    hipLaunchKernelGGL(frames_triang_finish_kernel, dim3(n), dim3(64), 0, s, a->D, b->D, dp, check_orientation ? 1 : 0, d_match12, d_nmatches);
    return kf_call_end(a);
}

int aos2_frames_fuse(aos2_frames_t *kfs, const aos2_map_points_dev_t *mps, int n_problems, int n_pts, const int32_t *target,
                     const int32_t *d_rows, float th, int32_t *d_best_idx, int32_t *d_best_dist)
{
    if (!kfs || !mps || n_problems <= 0 || n_pts <= 0 || !target || !d_rows || !d_best_idx || !d_best_dist || !kfs->dev_ready || !kfs->D.n ||
        !mps->normal || !mps->min_dist || !mps->max_dist) {
        set_error("bad argument (keyframe batch built; map points with normals and distance ranges)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(kfs->device);
    if (st) return st;
    for (int p = 0; p < n_problems; ++p)
        if (target[p] < 0 || target[p] >= kfs->D.batch) {
            set_error("problem %d names keyframe %d outside the batch", p, target[p]);
            return AOS2_ERR_ARG;
        }
    KfStage &stage = kfs->kf[kKfFuse];
    int32_t *h;
    if ((st = kf_stage_begin(stage, (size_t)n_problems, h))) return st;
    memcpy(h, target, 4 * (size_t)n_problems);
    const int32_t *d_target;
    if ((st = kf_stage_upload(kfs, stage, d_target))) return st;
    hipLaunchKernelGGL(frames_fuse_kernel, dim3((n_pts + 255) / 256, n_problems), dim3(256), 0, kfs->stream, kfs->D, map_points_dev(mps),
                       d_target, d_rows, n_pts, th, d_best_idx, d_best_dist);
    return kf_call_end(kfs);
}

int aos2_frames_set_async_keyframe_calls(aos2_frames_t *f, int on)
{
    if (!f) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    f->kf_async = on != 0;
    return AOS2_OK;
}

int aos2_frames_triangulate_matches(aos2_frames_t *a, aos2_frames_t *b, int n_pairs, const int32_t *kf1, const int32_t *kf2,
                                    const int32_t *d_match12, int first_wins, float *d_x3D, uint8_t *d_status, int32_t *d_nnew)
{
    if (!a || !b || n_pairs <= 0 || !kf1 || !kf2 || !d_match12 || !d_x3D || !d_status || !d_nnew || !a->dev_ready || !b->dev_ready || !a->D.n ||
        !b->D.n) {
        set_error("bad argument (both keyframe batches built)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(a->device);
    if (st) return st;
    const int n = n_pairs;
    for (int p = 0; p < n; ++p)
        if (kf1[p] < 0 || kf1[p] >= a->D.batch || kf2[p] < 0 || kf2[p] >= b->D.batch) {
            set_error("pair %d names keyframes (%d, %d) outside the batches", p, kf1[p], kf2[p]);
            return AOS2_ERR_ARG;
        }
    // staging (page-locked, then the handle's own device copy): kf1 | kf2 | group offsets | the pairs group by group
    const size_t words = 4 * (size_t)n + 1;
    KfStage &stage = a->kf[kKfNewPoints];
    int32_t *h;
    if ((st = kf_stage_begin(stage, words, h))) return st;
    int32_t *h_kf1 = h, *h_kf2 = h + n, *h_off = h + 2 * n, *h_grp;
    memcpy(h_kf1, kf1, 4 * (size_t)n);
    memcpy(h_kf2, kf2, 4 * (size_t)n);
    int n_groups = n;
    if (first_wins) {
        // one group per distinct kf1, in the order of first appearance; its pairs in call order
        std::vector<int32_t> group_of((size_t)a->D.batch, -1), count;
        for (int p = 0; p < n; ++p) {
            int32_t &g = group_of[kf1[p]];
            if (g < 0) {
                g = (int32_t)count.size();
                count.push_back(0);
            }
            ++count[g];
        }
        n_groups = (int)count.size();
        h_grp = h_off + n_groups + 1;
        h_off[0] = 0;
        for (int g = 0; g < n_groups; ++g) h_off[g + 1] = h_off[g] + count[g];
        std::fill(count.begin(), count.end(), 0);
        for (int p = 0; p < n; ++p) {
            const int g = group_of[kf1[p]];
            h_grp[h_off[g] + count[g]++] = p;
        }
    } else {
        h_grp = h_off + n_groups + 1;
        for (int p = 0; p < n; ++p) {
            h_off[p] = p;
            h_grp[p] = p;
        }
        h_off[n] = n;
    }
    hipStream_t s = a->stream;
    if (b != a && (st = order_behind(s, b))) return st;
    const int32_t *d;
    if ((st = kf_stage_upload(a, stage, d))) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(d_nnew, 0, 4 * (size_t)n, s));
    const int cap = a->D.cap;
    hipLaunchKernelGGL(frames_triangulate_kernel, dim3((cap + 255) / 256, n), dim3(256), 0, s, a->D, b->D, d, d + n, d_match12, d_x3D, d_status);
    hipLaunchKernelGGL(frames_triangulate_resolve_kernel, dim3((cap + 255) / 256, n_groups), dim3(256), 0, s, cap, d + 2 * n,
                       d + 2 * n + n_groups + 1, d_status, d_nnew);
    return kf_call_end(a);
}

}  // extern "C"
