// The planner's visibility count (camera::countVisible src/camera.cc:135-198 over camera::isInFrustum :263-315) on the device:
// the planner's map resident in HBM, and the counts of a batch of robot states in one call -- with what the planner forms from
// them, StateValidChecker::MotionCostCamera (src/StateValidChecker.cc:531-541) and plan_slam::AdvanceStepCamera (src/plan.cc:141-151).
//
// The result equals the reference's serial loop bit for bit, and num_visible is a FLOAT sum in point order, so the work is split
// into the part that is independent per (state, point) and the part that is ordered:
//   k_vis_setup   a lane per state: T_sc = T_sw * T_wb * T_bc and T_cs = T_sc.inverse() (:142-149 / :177-181)
//   k_vis_gate    a workgroup per (tile of states, group of points): a lane keeps its points in registers and walks the tile's
//                 states, whose matrices are wave-uniform (scalar loads); the ballot of 64 points is one mask word
//   k_vis_fold    a wave per state: the mask words in order, zero words skipped, the ratios of the set bits added lowest first
//   k_vis_costs   a lane per motion over the counts;  k_vis_advance  a wave over the counts of one trajectory
// The arithmetic is csrc/visibility.h, shared with aos2_debug_visibility_host (csrc/debug_taps.hip).
#include <cmath>
#include <vector>

#include "aos2_common.h"
#include "visibility.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kNT = 256;              // threads of every workgroup here
constexpr int kWaves = kNT / 64;
constexpr int kChunksPerWave = 2;     // 64-point chunks a wave of k_vis_gate keeps in registers: a state's 14 scalars serve 128 points
constexpr int kPointsPerWG = kWaves * kChunksPerWave * 64;
constexpr int kStateTile = 32;        // states a workgroup of k_vis_gate walks: one state against 10^5 points is still 196 workgroups
constexpr int kFoldGroup = 8;          // mask words whose ratios k_vis_fold loads together
constexpr int kMaxPoints = 65535 * kPointsPerWG;   // (the point groups are the grid's y)
enum { kX, kY, kZ, kUpper, kLower, kMaxRange, kMinRange, kRatio, kPlanes };

__global__ __launch_bounds__(kNT) void k_vis_setup(aos2_vis_camera_t cam, const float *__restrict__ in, int ns, int poses,
                                                   VisState *__restrict__ S)
{
    const int i = blockIdx.x * kNT + threadIdx.x;
    if (i >= ns) return;
    S[i] = poses ? vis_state_from_pose(in + 16 * (size_t)i, cam) : vis_state_from_xyt(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2], cam);
}

// map: kPlanes planes of n floats.  mask [ns][words], words = ceil(n / 64): every word of the tile's states and the group's
// chunks is written, also when it is zero.
__global__ __launch_bounds__(kNT) void k_vis_gate(VisGates g, const float *__restrict__ map, int n, int words,
                                                  const VisState *__restrict__ S, int ns, uint64_t *__restrict__ mask)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk0 = (blockIdx.y * kWaves + wave) * kChunksPerWave;   // wave-uniform
    float p[kChunksPerWave][kPlanes];
    bool in[kChunksPerWave];
#pragma unroll
    for (int c = 0; c < kChunksPerWave; ++c) {
        const int i = (chunk0 + c) * 64 + lane;
        in[c] = i < n;
#pragma unroll
        for (int k = 0; k < kPlanes; ++k) p[c][k] = in[c] ? map[(size_t)k * n + i] : 0.0f;
    }
    const int s0 = blockIdx.x * kStateTile, s1 = min(s0 + kStateTile, ns);
    for (int s = s0; s < s1; ++s) {
        const VisState st = S[s];
#pragma unroll
        for (int c = 0; c < kChunksPerWave; ++c) {
            if (chunk0 + c >= words) break;
            const bool pass = in[c] && vis_point(g, st, p[c][kX], p[c][kY], p[c][kZ], p[c][kUpper], p[c][kLower], p[c][kMaxRange], p[c][kMinRange]);
            const unsigned long long m = __ballot(pass);
            if (lane == 0) mask[(size_t)s * words + chunk0 + c] = m;
        }
    }
}

// the mask word that lane `src` (wave-uniform) holds as two halves, wave-uniform
__device__ __forceinline__ unsigned long long word_of(int lo, int hi, int src)
{
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(hi, src) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, src);
}

// num_visible += foundRatio[i] in point order (:153-160) and int(round(num_visible)) (:166)
__global__ __launch_bounds__(kNT) void k_vis_fold(const uint64_t *__restrict__ mask, int words, const float *__restrict__ ratio, int n,
                                                  int ns, float *__restrict__ sum, int32_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform
    if (s >= ns) return;
    const uint64_t *row = mask + (size_t)s * words;
    float acc = 0.0f;
    for (int base = 0; base < words; base += 64) {
        const int w = base + lane;
        const uint64_t m = w < words ? row[w] : 0ull;
        const unsigned long long nz = __ballot(m != 0);
        if (nz == 0) continue;
        // kFoldGroup words at a time: their ratio loads are issued together and waited for once -- with one load per word in
        // front of that word's additions, a state that sees thousands of points paid a memory round trip per word
        const int mlo = (int)(uint32_t)m, mhi = (int)(uint32_t)(m >> 32);
#pragma unroll 1
        for (int g = 0; g < 64; g += kFoldGroup) {
            if (((nz >> g) & ((1ull << kFoldGroup) - 1)) == 0) continue;   // wave-uniform
            float r[kFoldGroup];
#pragma unroll
            for (int k = 0; k < kFoldGroup; ++k) {
                const int i = (base + g + k) * 64 + lane;
                r[k] = (((word_of(mlo, mhi, g + k) >> lane) & 1ull) && i < n) ? ratio[i] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < kFoldGroup; ++k) {
                unsigned long long left = word_of(mlo, mhi, g + k);   // (read again instead of held in scalar registers over the loads)
                while (left) {   // word order, then lane order = point order: the reference's order of additions
                    const int b = __builtin_amdgcn_readfirstlane(__builtin_ctzll(left));
                    acc += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r[k]), b));
                    left &= left - 1;
                }
            }
        }
    }
    if (lane == 0) {
        sum[s] = acc;
        count[s] = vis_round(acc);
    }
}

// C += c < feature_threshold ? 1./1e-4 : 1./(double)c over the interior states of a motion, in index order
__global__ __launch_bounds__(kNT) void k_vis_costs(const int32_t *__restrict__ count, const int32_t *__restrict__ off, int nm, int thr,
                                                   double *__restrict__ cost)
{
    const int m = blockIdx.x * kNT + threadIdx.x;
    if (m >= nm) return;
    double C = 0;
    for (int i = off[m]; i < off[m + 1]; ++i) C += vis_motion_cost_term(count[i], thr);
    cost[m] = C;
}

// while (i < M.size() && count > thres) i++; i--;  one wave: the first failing state from the ballots
__global__ __launch_bounds__(64) void k_vis_advance(const int32_t *__restrict__ count, int ns, int thr, int32_t *__restrict__ index)
{
    const int lane = threadIdx.x;
    int first = ns;
    for (int base = 0; base < ns; base += 64) {
        const int i = base + lane;
        const unsigned long long fails = __ballot(i < ns && !(count[i] > thr));
        if (fails) {
            first = base + __builtin_ctzll(fails);
            break;
        }
    }
    if (lane == 0) *index = first - 1;
}

}  // namespace

struct aos2_vis {
    int device = 0;
    aos2_vis_camera_t cam;
    int n = 0;
    std::vector<float> map;     // kPlanes planes of n floats: the host copy (the host tap reads it)
    bool map_dirty = true;
    bool dev_ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    DevBuf<float> d_map, d_in, d_sum;
    DevBuf<VisState> d_states;
    DevBuf<uint64_t> d_mask;
    DevBuf<int32_t> d_count, d_off;
    DevBuf<double> d_cost;
    float last_ms = 0;
};

namespace aos2 {

void vis_view(const aos2_vis_t *h, aos2_vis_camera_t *cam, VisMapView *map)
{
    *cam = h->cam;
    const float *p = h->map.data();
    const size_t n = (size_t)h->n;
    map->n = h->n;
    map->x = p + kX * n; map->y = p + kY * n; map->z = p + kZ * n;
    map->upper = p + kUpper * n; map->lower = p + kLower * n;
    map->max_range = p + kMaxRange * n; map->min_range = p + kMinRange * n;
    map->ratio = p + kRatio * n;
}

int vis_check_count(const aos2_vis_t *h, int ns, const float *states, const int32_t *count)
{
    if (!h || ns < 0 || (ns > 0 && (!states || !count))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return AOS2_OK;
}

int vis_check_motions(const aos2_vis_t *h, int nm, const int32_t *offsets, const float *states, const double *cost)
{
    if (!h || nm < 0 || !offsets || (nm > 0 && (!states || !cost))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (offsets[0] != 0) {
        set_error("visibility: offsets start at %d", offsets[0]);
        return AOS2_ERR_ARG;
    }
    for (int m = 0; m < nm; ++m)
        if (offsets[m + 1] <= offsets[m]) {
            set_error("visibility: motion %d has %d states (an empty motion underflows Q.size()-1 in the reference)", m,
                      offsets[m + 1] - offsets[m]);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

int vis_check_advance(const aos2_vis_t *h, int ns, const float *states, const int32_t *index)
{
    if (!h || ns < 0 || !index || (ns > 0 && !states)) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return AOS2_OK;
}

void vis_interior(int nm, const int32_t *offsets, const float *states, std::vector<float> &packed, std::vector<int32_t> &packed_off)
{
    packed.clear();
    packed_off.assign(1, 0);
    for (int m = 0; m < nm; ++m) {
        for (int i = offsets[m] + 1; i < offsets[m + 1] - 1; ++i) packed.insert(packed.end(), states + 3 * (size_t)i, states + 3 * (size_t)i + 3);
        packed_off.push_back((int32_t)(packed.size() / 3));
    }
}

}  // namespace aos2

namespace {

int init_device(aos2_vis *h)
{
    if (int st = bind_device(h->device)) return st;
    if (h->dev_ready) return AOS2_OK;
    if (int st = stream_create(&h->stream, false)) return st;
    for (auto &e : h->ev) AOS2_HIP_CHECK(hipEventCreate(&e));
    h->dev_ready = true;
    return AOS2_OK;
}

// the handle's map into HBM on stream s, if it changed since the last upload
int upload_map(aos2_vis *h, hipStream_t s)
{
    if (!h->map_dirty) return AOS2_OK;
    if (int st = h->d_map.alloc(h->map.size())) return st;
    if (!h->map.empty()) AOS2_HIP_CHECK(hipMemcpyAsync(h->d_map.p, h->map.data(), h->map.size() * sizeof(float), hipMemcpyHostToDevice, s));
    h->map_dirty = false;
    return AOS2_OK;
}

// what the three kernels write for ns states
int alloc_counts(aos2_vis *h, int ns)
{
    int st;
    const int words = (h->n + 63) / 64;
    if ((st = h->d_states.alloc(ns)) || (st = h->d_mask.alloc((size_t)ns * words)) || (st = h->d_sum.alloc(ns)) || (st = h->d_count.alloc(ns)))
        return st;
    return AOS2_OK;
}

// the three kernels over ns states that are on the device already: `in` [ns][3] states or, with poses, [ns][16] matrices
int run_counts(aos2_vis *h, int ns, const float *in, bool poses, hipStream_t s)
{
    const int n = h->n, words = (n + 63) / 64;
    hipLaunchKernelGGL(k_vis_setup, dim3((ns + kNT - 1) / kNT), dim3(kNT), 0, s, h->cam, in, ns, poses ? 1 : 0, h->d_states.p);
    AOS2_HIP_CHECK(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(k_vis_gate, dim3((ns + kStateTile - 1) / kStateTile, (n + kPointsPerWG - 1) / kPointsPerWG), dim3(kNT), 0, s,
                           vis_gates(h->cam), h->d_map.p, n, words, h->d_states.p, ns, h->d_mask.p);
        AOS2_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_vis_fold, dim3((ns + kWaves - 1) / kWaves), dim3(kNT), 0, s, h->d_mask.p, words, h->d_map.p + (size_t)kRatio * n, n,
                       ns, h->d_sum.p, h->d_count.p);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

// The counts of ns states into d_sum / d_count, between the handle's two events (the caller records the second one, after the
// kernels it adds).  `in`: [ns][3] states or, with poses, [ns][16] matrices, host memory that outlives the stream's next wait.
int launch_counts(aos2_vis *h, int ns, const float *in, bool poses)
{
    int st;
    if ((st = init_device(h))) return st;
    hipStream_t s = h->stream;
    if ((st = upload_map(h, s))) return st;
    const size_t per = poses ? 16 : 3;
    if ((st = h->d_in.alloc(per * ns)) || (st = alloc_counts(h, ns))) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(h->d_in.p, in, per * ns * sizeof(float), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipEventRecord(h->ev[0], s));
    return run_counts(h, ns, h->d_in.p, poses, s);
}

int finish(aos2_vis *h)
{
    AOS2_HIP_CHECK(hipStreamSynchronize(h->stream));
    AOS2_HIP_CHECK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
    return AOS2_OK;
}

int count(aos2_vis *h, int ns, const float *in, bool poses, int32_t *cnt, float *sum, uint64_t *mask)
{
    if (int st = vis_check_count(h, ns, in, cnt)) return st;
    if (ns == 0) return AOS2_OK;
    if (int st = launch_counts(h, ns, in, poses)) return st;
    hipStream_t s = h->stream;
    const size_t words = (size_t)(h->n + 63) / 64;
    AOS2_HIP_CHECK(hipEventRecord(h->ev[1], s));
    AOS2_HIP_CHECK(hipMemcpyAsync(cnt, h->d_count.p, ns * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (sum) AOS2_HIP_CHECK(hipMemcpyAsync(sum, h->d_sum.p, ns * sizeof(float), hipMemcpyDeviceToHost, s));
    if (mask && words) AOS2_HIP_CHECK(hipMemcpyAsync(mask, h->d_mask.p, ns * words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    return finish(h);
}

}  // namespace

namespace aos2 {

int vis_counts_on_device(aos2_vis_t *h, int ns, const float *d_states, hipStream_t s, const int32_t **count)
{
    int st;
    if ((st = init_device(h)) || (st = upload_map(h, s)) || (st = alloc_counts(h, ns)) || (st = run_counts(h, ns, d_states, false, s))) return st;
    *count = h->d_count.p;
    return AOS2_OK;
}

}  // namespace aos2

extern "C" {

int aos2_vis_camera_default(int which, aos2_vis_camera_t *cam)
{
    if (!cam || (which != AOS2_VIS_CAMERA_MAP && which != AOS2_VIS_CAMERA_PLAIN)) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    const bool with_map = which == AOS2_VIS_CAMERA_MAP;
    cam->fx = 520.49f; cam->fy = 522.47f; cam->cx = 474.95f; cam->cy = 264.27f;
    cam->max_x = with_map ? 930.0f : 950.0f;
    cam->min_x = 10.0f;
    cam->max_y = with_map ? 520.0f : 530.0f;
    cam->min_y = with_map ? 20.0f : 10.0f;
    cam->max_dist = 6.0f;
    cam->min_dist = with_map ? 0.5f : 0.1f;
    cam->feature_threshold = 20;
    const float T_sw[16] = {0, -1.0f, 0, -0.1f, 0, 0, -1.0f, 0, 1.0f, 0, 0, -0.25f, 0, 0, 0, 1.0f};
    const float T_bc[16] = {0, 0, 1.0f, 0.25f, -1.0f, 0, 0, -0.1f, 0, -1.0f, 0, 0, 0, 0, 0, 1.0f};
    std::copy(T_sw, T_sw + 16, cam->T_sw);
    std::copy(T_bc, T_bc + 16, cam->T_bc);
    return AOS2_OK;
}

int aos2_vis_create(int device, aos2_vis_t **out)
{
    if (!out) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    aos2_vis *h = new aos2_vis();
    h->device = device;
    aos2_vis_camera_default(AOS2_VIS_CAMERA_MAP, &h->cam);
    *out = h;
    return AOS2_OK;
}

void aos2_vis_destroy(aos2_vis_t *h)
{
    if (!h) return;
    if (h->dev_ready) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        h->d_map.release(); h->d_in.release(); h->d_sum.release(); h->d_states.release(); h->d_mask.release();
        h->d_count.release(); h->d_off.release(); h->d_cost.release();
        for (auto &e : h->ev) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

int aos2_vis_set_camera(aos2_vis_t *h, const aos2_vis_camera_t *cam)
{
    if (!h || !cam) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    const float c[10] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->min_x, cam->max_x, cam->min_y, cam->max_y, cam->max_dist, cam->min_dist};
    bool finite = true;
    for (float v : c) finite = finite && std::isfinite(v);
    for (int i = 0; i < 16; ++i) finite = finite && std::isfinite(cam->T_sw[i]) && std::isfinite(cam->T_bc[i]);
    if (!finite) {
        set_error("visibility: a camera constant is not finite");
        return AOS2_ERR_ARG;
    }
    h->cam = *cam;
    return AOS2_OK;
}

int aos2_vis_set_map(aos2_vis_t *h, int n, const float *xyz, const float *upper, const float *lower, const float *max_range,
                     const float *min_range, const float *found_ratio)
{
    if (!h || n < 0 || n > kMaxPoints || (n > 0 && (!xyz || !upper || !lower || !max_range || !min_range || !found_ratio))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (h->dev_ready) {   // (a call's copies are waited for before it returns; this is for a call that failed half way)
        if (int st = bind_device(h->device)) return st;
        AOS2_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    const size_t N = (size_t)n;
    h->map.resize(kPlanes * N);
    float *p = h->map.data();
    for (size_t i = 0; i < N; ++i) {
        p[kX * N + i] = xyz[3 * i];
        p[kY * N + i] = xyz[3 * i + 1];
        p[kZ * N + i] = xyz[3 * i + 2];
    }
    if (n) {
        std::copy(upper, upper + N, p + kUpper * N);
        std::copy(lower, lower + N, p + kLower * N);
        std::copy(max_range, max_range + N, p + kMaxRange * N);
        std::copy(min_range, min_range + N, p + kMinRange * N);
        std::copy(found_ratio, found_ratio + N, p + kRatio * N);
    }
    h->n = n;
    h->map_dirty = true;
    return AOS2_OK;
}

int aos2_vis_map_size(const aos2_vis_t *h) { return h ? h->n : 0; }

void aos2_vis_gate_tile(int *points, int *states)
{
    if (points) *points = kPointsPerWG;
    if (states) *states = kStateTile;
}

int aos2_vis_count(aos2_vis_t *h, int ns, const float *states, int32_t *cnt, float *sum, uint64_t *mask)
{
    return count(h, ns, states, false, cnt, sum, mask);
}

int aos2_vis_count_poses(aos2_vis_t *h, int ns, const float *T_wb, int32_t *cnt, float *sum, uint64_t *mask)
{
    return count(h, ns, T_wb, true, cnt, sum, mask);
}

int aos2_vis_motion_costs(aos2_vis_t *h, int nm, const int32_t *offsets, const float *states, int thres, double *cost)
{
    if (int st = vis_check_motions(h, nm, offsets, states, cost)) return st;
    if (nm == 0) return AOS2_OK;
    std::vector<float> packed;
    std::vector<int32_t> off;
    vis_interior(nm, offsets, states, packed, off);
    const int ns = off[nm];
    if (ns == 0) {   // no motion has an interior state
        std::fill(cost, cost + nm, 0.0);
        return AOS2_OK;
    }
    int st;
    if ((st = launch_counts(h, ns, packed.data(), false)) || (st = h->d_off.alloc(nm + 1)) || (st = h->d_cost.alloc(nm))) return st;
    hipStream_t s = h->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(h->d_off.p, off.data(), (nm + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_vis_costs, dim3((nm + kNT - 1) / kNT), dim3(kNT), 0, s, h->d_count.p, h->d_off.p, nm,
                       thres < 0 ? h->cam.feature_threshold : thres, h->d_cost.p);
    AOS2_HIP_CHECK(hipGetLastError());
    AOS2_HIP_CHECK(hipEventRecord(h->ev[1], s));
    AOS2_HIP_CHECK(hipMemcpyAsync(cost, h->d_cost.p, nm * sizeof(double), hipMemcpyDeviceToHost, s));
    return finish(h);   // (packed and off are read by copies on the stream: they live until this wait)
}

int aos2_vis_advance(aos2_vis_t *h, int ns, const float *states, int thres, int32_t *index)
{
    if (int st = vis_check_advance(h, ns, states, index)) return st;
    if (ns == 0) {
        *index = -1;
        return AOS2_OK;
    }
    int st;
    if ((st = launch_counts(h, ns, states, false)) || (st = h->d_off.alloc(1))) return st;
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(k_vis_advance, dim3(1), dim3(64), 0, s, h->d_count.p, ns, thres == -1 ? h->cam.feature_threshold : thres, h->d_off.p);
    AOS2_HIP_CHECK(hipGetLastError());
    AOS2_HIP_CHECK(hipEventRecord(h->ev[1], s));
    AOS2_HIP_CHECK(hipMemcpyAsync(index, h->d_off.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return finish(h);
}

float aos2_vis_last_device_ms(const aos2_vis_t *h) { return h ? h->last_ms : 0.0f; }

}  // extern "C"
