// Device-resident batches of Frames (src/Frame.cc) and the MapPoint table they reference: the members the per-frame
// tracking path reads and writes, kept in HBM between the calls of the chain
//   ORBextractor::operator() -> Frame::Frame (stereo from RGB-D, grid) -> SearchByProjection(Current, Last)
//   -> PoseOptimization -> SearchLocalPoints (isInFrustum + SearchByProjection(F, vpMapPoints)) -> PoseOptimization
// so that no keypoint, descriptor, match or pose crosses PCIe between them.  Internal to the library; the public
// entry points are the aos2_frames_* functions of include/aos2.h.  Their translation units: frames.hip (lifetime, build,
// the two searches of the chain), frames_keyframe.hip (SearchForTriangulation, Fuse, CreateNewMapPoints), frames_pose.hip
// (PoseOptimization), local_map.hip (UpdateLocalMap).  This header is what they share: the batch and its handle, frame_of
// (one frame as search_device.h's routines take it) and, at the end, the host steps more than one of them runs.
#pragma once
#include "aos2_common.h"
#include "regions.h"
#include "search_device.h"

namespace aos2 {

constexpr int kFrGridCols = AOS2_GRID_COLS, kFrGridRows = AOS2_GRID_ROWS, kFrGridCells = kFrGridCols * kFrGridRows;

// [B][cap] arrays unless noted
struct FramesDev {
    int batch, cap, n_levels;
    const int32_t *n;              // [B] Frame::N
    const aos2_keypoint_t *kps;    // mvKeys (the extractor's output, borrowed)
    const uint8_t *desc;           // [B][cap][32] mDescriptors (borrowed)
    float *kp_x, *kp_y, *kp_angle; // mvKeysUn[i].pt / .angle
    int32_t *kp_octave;            // mvKeysUn[i].octave
    float *u_right, *depth;        // mvuRight, mvDepth
    int32_t *grid_off, *grid_idx;  // mGrid[64][48] as CSR: [B][64 * 48 + 1], [B][cap]
    int32_t *mp;                   // mvpMapPoints as indices into the map-point table, -1 = NULL
    int32_t *mp_seen;              // map point taken away as an outlier in this frame (mnLastFrameSeen = this frame), -1 = none
    uint8_t *mp_state;             // 0 = NULL, 1 = map point without observations, 2 = Observations() > 0
    uint8_t *outlier;              // mvbOutlier
    float *Tcw;                    // [B][16] mTcw, row-major
    const float *scale_factors, *inv_level_sigma2;   // [n_levels] mvScaleFactors, mvInvLevelSigma2
    float min_x, min_y, max_x, max_y, grid_w_inv, grid_h_inv;   // mnMinX .. mfGridElementHeightInv
    float fx, fy, cx, cy, mb, mbf, log_scale_factor;
    float dist[5];                 // mDistCoef: k1 k2 p1 p2 k3 (all 0: mvKeysUn = mvKeys)
    int has_dist;                  // mDistCoef.at<float>(0) != 0 (the reference's test, src/Frame.cc:435)
};

// frame b of a batch as the searches see one frame (search_device.h)
__device__ __forceinline__ FrameDev frame_of(const FramesDev &S, int b)
{
    FrameDev F;
    const size_t o = (size_t)b * S.cap;
    F.n_f = S.n[b];
    F.n_levels = S.n_levels;
    F.desc_f = S.desc + o * 32;
    F.kp_x = S.kp_x + o;
    F.kp_y = S.kp_y + o;
    F.kp_angle = S.kp_angle + o;
    F.u_right = S.u_right + o;
    F.scale_factors = S.scale_factors;
    F.kp_octave = S.kp_octave + o;
    F.min_x = S.min_x; F.min_y = S.min_y; F.max_x = S.max_x; F.max_y = S.max_y;
    F.grid_w_inv = S.grid_w_inv; F.grid_h_inv = S.grid_h_inv;
    F.grid_off = S.grid_off + (size_t)b * (kFrGridCells + 1);
    F.grid_idx = S.grid_idx + o;
    F.f_mp_state = S.mp_state + o;
    return F;
}

// the members of MapPoint the per-frame path reads (include/MapPoint.h): GetWorldPos, GetDescriptor, Observations() > 0,
// GetNormal, mfMinDistance / mfMaxDistance (raw)
// cv::undistortPoints(p, p, K, distCoef, noArray(), K) on one CV_32FC2 point, as Frame::UndistortKeyPoints /
// Frame::ComputeImageBounds use it (src/Frame.cc:433-493).  OpenCV 3.2 imgproc/undistort.cpp, cvUndistortPoints: camera
// matrix and coefficients widened to double, 5 fixed-point iterations of the inverse of the radial (k1 k2 k3) +
// tangential (p1 p2) model, then P R = K applied, the result rounded to float.  The operation sequence is the library's
// (the terms of the unused higher-order coefficients are kept as products with 0: they decide the sign of a zero); host
// and device run this same function (-ffp-contract=off).
__host__ __device__ inline void undistort_point(float fx_f, float fy_f, float cx_f, float cy_f, const float *k_f, float xin, float yin,
                                                float &xout, float &yout)
{
    const double fx = (double)fx_f, fy = (double)fy_f, cx = (double)cx_f, cy = (double)cy_f;
    const double ifx = 1. / fx, ify = 1. / fy;
    const double k0 = (double)k_f[0], k1 = (double)k_f[1], k2 = (double)k_f[2], k3 = (double)k_f[3], k4 = (double)k_f[4];
    double x = ((double)xin - cx) * ifx, y = ((double)yin - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((0. * r2 + 0.) * r2 + 0.) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        const double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x) + 0. * r2 + 0. * r2 * r2;
        const double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y + 0. * r2 + 0. * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = fx * x + 0. * y + cx;
    const double yy = 0. * x + fy * y + cy;
    const double ww = 1. / (0. * x + 0. * y + 1.);
    xout = (float)(xx * ww);
    yout = (float)(yy * ww);
}

struct MapPointsDev {
    int n;
    const float *pos;        // n x 3
    const uint8_t *desc;     // n x 32
    const uint8_t *has_obs;  // n
    const float *normal;     // n x 3
    const float *min_dist, *max_dist;   // n
};

inline MapPointsDev map_points_dev(const aos2_map_points_dev_t *t)
{
    MapPointsDev M;
    M.n = t->n; M.pos = t->pos; M.desc = t->desc; M.has_obs = t->has_obs; M.normal = t->normal;
    M.min_dist = t->min_dist; M.max_dist = t->max_dist;
    return M;
}

// Staging of one kind of keyframe call: what the host assembles, page-locked, and its device copy, both kept by the handle.
// `uploaded` lies behind the last upload (created by the first asynchronous call): the host buffer is rewritten only after it.
struct KfStage {
    PinnedBuf<uint8_t> host;
    DevBuf<uint8_t> dev;
    size_t bytes = 0;   // what the call in progress stages: fixed when its buffers are sized, uploaded as that
    hipEvent_t uploaded = nullptr;
};
enum { kKfTriang, kKfFuse, kKfNewPoints, kKfKinds };   // SearchForTriangulation, Fuse, TriangulateMatches

}  // namespace aos2

struct aos2_frames {
    int device = 0;
    bool dev_ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t order_ev = nullptr;   // ordering only (no timing): recorded on this batch's stream for a batch that reads its members
    hipEvent_t ext_ev = nullptr;     // recorded on a caller's stream by aos2_frames_wait_for_stream
    aos2::FramesDev D = {};
    int32_t *d_overflow = nullptr;   // sticky: largest per-frame window population that exceeded the entry pool's share
    aos2::DevBuf<uint8_t> mem;       // the per-frame member arrays
    aos2::DevBuf<float> tables;      // scale factors | inverse level sigma2
    aos2::PinnedBuf<float> h_tables; // ... as aos2_frames_build assembles them
    // scratch of the searches that run on this batch (sized at the first use)
    aos2::DevBuf<uint8_t> scratch;
    aos2::DevBuf<uint64_t> pool;     // candidate entries (8 B each)
    aos2::DevBuf<uint8_t> pose_mem;  // PoseOptimization problem arrays
    aos2::PinnedBuf<int32_t> h_overflow;   // d_overflow: written by the kernels, read by aos2_frames_wait
    aos2::KfStage kf[aos2::kKfKinds];   // one slot per kind: a handle's SearchForTriangulation, Fuse and TriangulateMatches may all be in flight
    bool kf_async = false;              // aos2_frames_set_async_keyframe_calls: the keyframe entry points return after enqueueing
    float dist[5] = {0, 0, 0, 0, 0};   // mDistCoef for the next aos2_frames_build (aos2_frames_set_distortion)
};

namespace aos2 {

// binds the batch's device and, on the first call, creates its stream and member arrays (csrc/frames.hip)
int frames_init(aos2_frames *f);

// `s` waits for everything enqueued on the producer batch's stream so far: the kernels the caller puts on `s` read members
// (mvpMapPoints, mvbOutlier, mTcw, keys) that the work on the producer's own stream may still be writing -- in a tracking loop
// the previous CurrentFrame batch becomes LastFrame while its PoseOptimization is in flight.  The entry points take the
// producer as a read-only batch; the event it lends to the ordering is the handle's bookkeeping, none of its members: hence
// the const_cast, here and nowhere else.
inline int order_behind(hipStream_t s, const aos2_frames *producer)
{
    aos2_frames *p = const_cast<aos2_frames *>(producer);
    if (!p->order_ev) AOS2_HIP_CHECK(hipEventCreateWithFlags(&p->order_ev, hipEventDisableTiming));
    AOS2_HIP_CHECK(hipEventRecord(p->order_ev, p->stream));
    AOS2_HIP_CHECK(hipStreamWaitEvent(s, p->order_ev, 0));
    return AOS2_OK;
}

// A keyframe call stages its host arrays through its slot of the batch: kf_stage_begin, the host fill, (order_behind,)
// kf_stage_upload, the kernels, kf_call_end.
//
// the slot's last upload is over (asynchronous calls), both buffers hold `count` elements -> the page-locked one, to be filled
template <class T>
inline int kf_stage_begin(KfStage &k, size_t count, T *&host)
{
    if (k.uploaded) AOS2_HIP_CHECK(hipEventSynchronize(k.uploaded));
    k.bytes = sizeof(T) * count;
    if (int st = k.host.alloc(k.bytes)) return st;
    if (int st = k.dev.alloc(k.bytes)) return st;
    host = reinterpret_cast<T *>(k.host.p);
    return AOS2_OK;
}

// the filled buffer goes to the device on the batch's stream -> its device copy; an asynchronous call marks the upload's end
template <class T>
inline int kf_stage_upload(aos2_frames *f, KfStage &k, const T *&dev)
{
    AOS2_HIP_CHECK(hipMemcpyAsync(k.dev.p, k.host.p, k.bytes, hipMemcpyHostToDevice, f->stream));
    if (f->kf_async) {
        if (!k.uploaded) AOS2_HIP_CHECK(hipEventCreateWithFlags(&k.uploaded, hipEventDisableTiming));
        AOS2_HIP_CHECK(hipEventRecord(k.uploaded, f->stream));
    }
    dev = reinterpret_cast<const T *>(k.dev.p);
    return AOS2_OK;
}

// the kernels are enqueued: a synchronous call waits for them, an asynchronous one leaves that to aos2_frames_wait
inline int kf_call_end(aos2_frames *f)
{
    AOS2_HIP_CHECK(hipGetLastError());
    if (!f->kf_async) AOS2_HIP_CHECK(hipStreamSynchronize(f->stream));
    return AOS2_OK;
}

}  // namespace aos2
