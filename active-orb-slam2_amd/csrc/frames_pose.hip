// Optimizer::PoseOptimization over a device-resident frame batch (include/aos2.h: aos2_frames_pose_optimization) around
// pose_optimization_body of pose_opt.h.  The gather is the edge-building loop of src/Optimizer.cc:260-350 on the device:
// the features that hold a map point, in feature order; mono edge when mvuRight < 0, stereo edge otherwise.
#include "frames.h"
#include "pose_opt.h"

namespace aos2 {

struct PoseBatchDev {
    float *Xw, *obs, *w;     // [B][cap] x 3, 3, 1
    double *err;             // [B][cap]
    uint8_t *stereo, *l1, *rb, *out;   // [B][cap]
    int32_t *feat_of;        // [B][cap] feature index of correspondence k
    double *pose_out;        // [B][7]
    int32_t *counts;         // [B][2]
};

// One workgroup per frame: gather (feature -> correspondence, stable compaction by a workgroup scan), the solver
// (pose_optimization_body), scatter -- one launch instead of three.
template <int kEpt, int NT = 256>
__global__ __launch_bounds__(NT) void frames_pose_optimization_kernel(FramesDev S, MapPointsDev M, PoseBatchDev Q, int32_t *inliers)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];  // po_lds_bytes(NT)
    __shared__ int s_cnt;
    __shared__ int32_t wsum[NT / 64];
    __shared__ double s_pose[7];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)b * S.cap;
    const int n = S.n[b];
    if (tid == 0) {
        double qt[7];
        pose_from_Tcw(S.Tcw + 16 * (size_t)b, qt);
        for (int k = 0; k < 7; ++k) s_pose[k] = qt[k];
    }
    int carry = 0;   // correspondences of the chunks before this one (uniform)
    for (int i0 = 0; i0 < n; i0 += NT) {
        const int i = i0 + tid;
        const int row = i < n ? S.mp[o + i] : -1;
        const int v = row >= 0 ? 1 : 0;
        int total;
        const int k = carry + block_excl_scan_i32<NT>(v, wsum, total);
        if (v) {
            const size_t d = o + k;
            const float ur = S.u_right[o + i];
            for (int c = 0; c < 3; ++c) Q.Xw[3 * d + c] = M.pos[3 * (size_t)row + c];
            Q.obs[3 * d] = S.kp_x[o + i];
            Q.obs[3 * d + 1] = S.kp_y[o + i];
            Q.obs[3 * d + 2] = ur;
            Q.w[d] = S.inv_level_sigma2[S.kp_octave[o + i]];
            Q.stereo[d] = ur >= 0 ? 1 : 0;   // mvuRight[i] < 0 -> monocular observation (:275)
            Q.feat_of[d] = i;
            S.outlier[o + i] = 0;            // pFrame->mvbOutlier[i] = false (:283, :320)
        }
        carry += total;
        __syncthreads();   // wsum is read before the next chunk writes it
    }
    PoseProbDev P;
    P.n = carry;
    P.Xw = Q.Xw + 3 * o; P.obs = Q.obs + 3 * o; P.w = Q.w + o; P.stereo = Q.stereo + o;
    P.err = Q.err + o; P.level1 = Q.l1 + o; P.robust = Q.rb + o; P.outlier = Q.out + o;
    P.fx = (double)S.fx; P.fy = (double)S.fy; P.cx = (double)S.cx; P.cy = (double)S.cy; P.bf = (double)S.mbf;
#pragma unroll
    for (int k = 0; k < 7; ++k) P.pose_in[k] = s_pose[k];
    P.pose_out = Q.pose_out + 7 * (size_t)b;
    P.counts = Q.counts + 2 * (size_t)b;
    pose_optimization_body<kEpt, NT>(P, sh, &s_cnt);
    __syncthreads();
    // pFrame->SetPose(Converter::toCvMat(SE3quat_recov)) (:446-448), mvbOutlier, return nInitialCorrespondences - nBad
    const int nc = P.n;
    for (int k = tid; k < nc; k += NT) S.outlier[o + Q.feat_of[o + k]] = Q.out[o + k];
    if (tid == 0) {
        if (nc >= 3) pose_to_Tcw(P.pose_out, S.Tcw + 16 * (size_t)b);   // (n < 3: return 0 before the pose is touched, :355-356)
        if (inliers) inliers[b] = P.counts[1];
    }
}

}  // namespace aos2

extern "C" int aos2_frames_pose_optimization(aos2_frames_t *f, const aos2_map_points_dev_t *mps, int32_t *d_inliers)
{
    using namespace aos2;
    if (!f || !mps || !f->dev_ready || !f->D.n) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(f->device);
    if (st) return st;
    const size_t B = (size_t)f->D.batch, cap = (size_t)f->D.cap, n = B * cap;
    PoseBatchDev Q;
    Regions<11> R;
    R.add(Q.Xw, 3 * n); R.add(Q.obs, 3 * n); R.add(Q.w, n); R.add(Q.err, n);
    R.add(Q.stereo, n); R.add(Q.l1, n); R.add(Q.rb, n); R.add(Q.out, n); R.add(Q.feat_of, n); R.add(Q.pose_out, 7 * B); R.add(Q.counts, 2 * B);
    if ((st = f->pose_mem.alloc(R.bytes() + 256))) return st;
    R.bind(f->pose_mem.p);
    const MapPointsDev M = map_points_dev(mps);
    hipStream_t q = f->stream;
    const size_t po_lds = kPoLds;
    // 256 threads per frame, 4 edge slots per thread.  (512 threads x 2 slots and 1024 x 1 were measured -- the template
    // parameter NT exists for that: a shorter edge chain per pass, but the two barriers and the 8- / 16-wave sum of every pass
    // cost more than the chain saves: single frame 0.19 -> 0.21 ms with 512 threads; 1024 threads leave 128 registers per
    // thread and spill: 0.40 ms.  DESIGN.md section 5.6.)
    // Batches that do not fit the device at four waves per frame (one wave per SIMD: the kernel holds 256 + 61 registers) run 128 threads
    // per frame, 9 edge slots per thread: every frame of a 512-frame batch is resident at once instead of two rounds of 256 workgroups --
    // 0.45 -> 0.32 ms per call, although one frame alone takes longer that way (AOS2_PO_THREADS = 128 / 256 forces a form).
    static const int forced = getenv("AOS2_PO_THREADS") ? atoi(getenv("AOS2_PO_THREADS")) : 0;
    const bool narrow = forced ? forced == 128 : B > 256;
    if (narrow && cap <= 128 * 9)
        hipLaunchKernelGGL((frames_pose_optimization_kernel<9, 128>), dim3((unsigned)B), dim3(128), po_lds, q, f->D, M, Q, d_inliers);
    else if (cap <= 256 * 4)   // edges live in registers
        hipLaunchKernelGGL(frames_pose_optimization_kernel<4>, dim3((unsigned)B), dim3(256), po_lds, q, f->D, M, Q, d_inliers);
    else if (cap <= 256 * 8)
        hipLaunchKernelGGL(frames_pose_optimization_kernel<8>, dim3((unsigned)B), dim3(256), po_lds, q, f->D, M, Q, d_inliers);
    else
        hipLaunchKernelGGL(frames_pose_optimization_kernel<0>, dim3((unsigned)B), dim3(256), po_lds, q, f->D, M, Q, d_inliers);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}
