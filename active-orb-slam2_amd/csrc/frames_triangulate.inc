// The loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) on the device (include/aos2.h:
// aos2_frames_triangulate_matches, aos2_triangulate_matches), part of matcher.hip's translation unit next to the keyframe searches
// whose matches it consumes.  The arithmetic is csrc/triangulate.h, shared with the host tap.
#include "triangulate.h"

namespace aos2 {

// number of set bits of a ballot below this lane (v_mbcnt_lo + v_mbcnt_hi)
__device__ __forceinline__ int tri_lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One matched pair per thread of a 256-thread workgroup whose threads share (K1, K2); every thread of the workgroup calls it.
// The cheap part (rays, parallax, the choice of branch) runs where the match is.  Typically under a tenth of a keyframe's features
// are matched, and the Jacobi SVD is a few thousand f64 instructions: under the divergent `if` most lanes of all four waves would
// idle through it.  So the items that need it are compacted per workgroup (ballot + mbcnt, their xn in LDS), the first `total`
// threads run the SVD on dense lanes -- the sweep loop of a wave ends when none of its lanes rotated; a sweep on a converged lane
// changes nothing, so a lane's result does not depend on its neighbours -- and every item picks its vt.row(3) up again.
__device__ __forceinline__ int tri_block(bool matched, const TriKf &K1, const TriKf &K2, const TriObs &o1, const TriObs &o2, float x3D[3])
{
    __shared__ float s_v[4][256];
    __shared__ int s_wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float xn[4] = {0.f, 0.f, 0.f, 0.f};
    int branch = TRI_BRANCH_NONE;
    if (matched) branch = tri_front(K1, K2, o1, o2, xn);
    const bool need = branch == TRI_BRANCH_SVD;
    const unsigned long long bal = __ballot(need);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = s_wcnt[w];
        if (w < wave) base += c;
        total += c;
    }
    const int slot = base + tri_lanes_below(bal);   // < 256: at most one item per thread
    if (need) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_v[k][slot] = xn[k];
    }
    __syncthreads();
    if (tid < total) {
        float in[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) in[k] = s_v[k][tid];
        tri_svd_null(K1, K2, in, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_v[k][tid] = v[k];
    }
    __syncthreads();
    x3D[0] = x3D[1] = x3D[2] = 0.0f;
    if (!matched) return AOS2_TRI_NO_MATCH;
    if (branch == TRI_BRANCH_NONE) return AOS2_TRI_LOW_PARALLAX;
    if (need) {
        const float v[4] = {s_v[0][slot], s_v[1][slot], s_v[2][slot], s_v[3][slot]};
        if (!tri_dehomogenize(v, x3D)) return AOS2_TRI_W_ZERO;
    } else if (branch == TRI_BRANCH_STEREO1) {
        tri_unproject(K1, o1, x3D);
    } else {
        tri_unproject(K2, o2, x3D);
    }
    return tri_gates(K1, K2, o1, o2, x3D);
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

// the host-pointer form: one (KF1, KF2) pair, thread = match
__global__ __launch_bounds__(256) void triangulate_list_kernel(const aos2_triang_geom_t *__restrict__ G, int n, const aos2_triang_obs_t *__restrict__ obs1,
                                                              const aos2_triang_obs_t *__restrict__ obs2, float *__restrict__ x3D_out,
                                                              uint8_t *__restrict__ status_out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const TriKf K1 = {G->Tcw1, G->fx1, G->fy1, G->cx1, G->cy1, G->mb1, G->mbf1, G->scale_factors1};
    const TriKf K2 = {G->Tcw2, G->fx2, G->fy2, G->cx2, G->cy2, G->mb2, G->mbf2, G->scale_factors2};
    TriObs q1 = {}, q2 = {};
    if (k < n) {
        const aos2_triang_obs_t a = obs1[k], b = obs2[k];
        q1 = TriObs{a.ux, a.uy, a.kx, a.ky, a.u_right, a.depth, a.octave};
        q2 = TriObs{b.ux, b.uy, b.kx, b.ky, b.u_right, b.depth, b.octave};
    }
    float x3D[3];
    const int st = tri_block(k < n, K1, K2, q1, q2, x3D);
    if (k < n) {
        status_out[k] = (uint8_t)st;
        x3D_out[3 * (size_t)k] = x3D[0]; x3D_out[3 * (size_t)k + 1] = x3D[1]; x3D_out[3 * (size_t)k + 2] = x3D[2];
    }
}

}  // namespace aos2

extern "C" {

int aos2_frames_triangulate_matches(aos2_frames_t *a, aos2_frames_t *b, int n_pairs, const int32_t *kf1, const int32_t *kf2,
                                    const int32_t *d_match12, int first_wins, float *d_x3D, uint8_t *d_status, int32_t *d_nnew)
{
    using namespace aos2;
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

int aos2_triangulate_matches(aos2_matcher_t *m, const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1,
                             const aos2_triang_obs_t *obs2, float *x3D, uint8_t *status)
{
    using namespace aos2;
    if (!m) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = triang_check(g, n, obs1, obs2, x3D, status);
    if (st || n == 0) return st;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    const aos2_triang_geom_t *d_g;
    const aos2_triang_obs_t *d_o1, *d_o2;
    float *d_x;
    uint8_t *d_s;
    A.in(d_g, g, sizeof(*g));
    A.in(d_o1, obs1, sizeof(aos2_triang_obs_t) * (size_t)n);
    A.in(d_o2, obs2, sizeof(aos2_triang_obs_t) * (size_t)n);
    A.out(d_x, 12 * (size_t)n);
    A.out(d_s, (size_t)n);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(triangulate_list_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, d_g, n, d_o1, d_o2, d_x, d_s);
    A.fetch(x3D, d_x, 12 * (size_t)n);
    A.fetch(status, d_s, (size_t)n);
    return A.end();
}

}  // extern "C"
