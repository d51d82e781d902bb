// Optimizer::PoseOptimization on gfx950 (reference src/Optimizer.cc:239-452; g2o: types_six_dof_expmap.cpp:266-364,
// optimization_algorithm_levenberg.cpp:61-164, linear_solver_dense.h:64-110).  SURVEY.md section 8(f) rank 1.
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "lba_math.h"
#include "pose_opt.h"
#include "wave_ops.h"

namespace aos2 {

template <int kEpt>
__global__ __launch_bounds__(256) void pose_optimization_kernel(const PoseProbDev *__restrict__ probs)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];  // kPoLds
    __shared__ int s_cnt;
    const PoseProbDev P = probs[blockIdx.x];
    pose_optimization_body<kEpt>(P, sh, &s_cnt);
}

}  // namespace aos2

using namespace aos2;

extern "C" {

int aos2_pose_optimization(aos2_lba_t *s, const aos2_pose_problem_t *problems, aos2_pose_result_t *results, int n_problems)
{
    if (!s || !problems || !results || n_problems <= 0) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n_problems; ++i)
        if (problems[i].n < 0 || (problems[i].n > 0 && (!problems[i].Xw || !problems[i].obs || !problems[i].stereo ||
                                                        !problems[i].inv_sigma2 || !results[i].outlier))) {
            set_error("bad pose problem %d", i);
            return AOS2_ERR_ARG;
        }
    int st = lba_handle_init(s);
    if (st) return st;
    // Inputs are converted in place into the handle's page-locked staging buffer (one asynchronous upload that
    // also carries the problem descriptors); the results of all problems -- pose, counts, outlier flags -- are
    // neighbours in the arena and come back as ONE copy (the former three small pageable copies per problem cost
    // 2 ms of host time for 64 frames, against 0.55 ms of kernel).
    HostArena H;
    struct Off { size_t xw, obs, w, st, err, l1, rb, out, pose, cnt; };
    std::vector<Off> offs(n_problems);
    size_t in_cap = sizeof(PoseProbDev) * (size_t)n_problems + 512;
    for (int i = 0; i < n_problems; ++i) in_cap += (size_t)problems[i].n * (24 + 24 + 8 + 1) + 4 * 256 + 32;
    if ((st = s->h_in.alloc(in_cap))) return st;
    H.host = s->h_in.p;
    H.host_cap = in_cap;
    for (int i = 0; i < n_problems; ++i) {
        const aos2_pose_problem_t &p = problems[i];
        const size_t n = (size_t)p.n;
        float *xw = H.push_fill<float>(3 * n + 1, offs[i].xw), *ob = H.push_fill<float>(3 * n + 1, offs[i].obs);
        float *w = H.push_fill<float>(n + 1, offs[i].w);
        uint8_t *sv = H.push_fill<uint8_t>(n + 1, offs[i].st);
        if (!xw || !ob || !w || !sv) {
            set_error("internal: pose optimisation input staging");
            return AOS2_ERR_ARG;
        }
        if (n) {
            memcpy(xw, p.Xw, 12 * n);
            memcpy(ob, p.obs, 12 * n);
            memcpy(w, p.inv_sigma2, 4 * n);
            memcpy(sv, p.stereo, n);
        }
        xw[3 * n] = ob[3 * n] = w[n] = 0.f;
        sv[n] = 0;
    }
    size_t o_probs;
    PoseProbDev *dev = H.push_fill<PoseProbDev>((size_t)n_problems, o_probs);   // filled below (needs the device base)
    if (!dev) {
        set_error("internal: pose optimisation input staging");
        return AOS2_ERR_ARG;
    }
    const size_t in_bytes = H.host_size;
    for (int i = 0; i < n_problems; ++i) {
        const size_t n = (size_t)problems[i].n;
        offs[i].err = H.push(nullptr, (n + 1) * 8);
        offs[i].l1 = H.push(nullptr, n + 1);
        offs[i].rb = H.push(nullptr, n + 1);
    }
    const size_t o_res = (H.size + 255) & ~(size_t)255;   // results of all problems from here on
    for (int i = 0; i < n_problems; ++i) {
        offs[i].pose = H.push(nullptr, 7 * 8);
        offs[i].cnt = H.push(nullptr, 8);
        offs[i].out = H.push(nullptr, (size_t)problems[i].n + 1);
    }
    const size_t res_bytes = H.size - o_res;
    if ((st = s->arena.alloc(H.size + 256))) return st;
    if ((st = s->h_stage.alloc(res_bytes + 64))) return st;
    uint8_t *base = s->arena.p;
    for (int i = 0; i < n_problems; ++i) {
        const aos2_pose_problem_t &p = problems[i];
        PoseProbDev &D = dev[i];
        D.n = p.n;
        D.Xw = (const float *)(base + offs[i].xw); D.obs = (const float *)(base + offs[i].obs);
        D.w = (const float *)(base + offs[i].w); D.stereo = base + offs[i].st;
        D.err = (double *)(base + offs[i].err); D.level1 = base + offs[i].l1; D.robust = base + offs[i].rb;
        D.outlier = base + offs[i].out; D.pose_out = (double *)(base + offs[i].pose); D.counts = (int32_t *)(base + offs[i].cnt);
        D.fx = (double)p.fx; D.fy = (double)p.fy; D.cx = (double)p.cx; D.cy = (double)p.cy; D.bf = (double)p.bf;
        pose_from_Tcw(p.Tcw, D.pose_in);
    }
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(base, H.data(), in_bytes, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipEventRecord(s->ev[0], q));
    int max_n = 0;
    for (int i = 0; i < n_problems; ++i) max_n = std::max(max_n, problems[i].n);
    const size_t po_lds = kPoLds;
    if (max_n <= 256 * 4)   // the usual case (a frame has <= ~1000 map-point matches): edges live in registers
        hipLaunchKernelGGL(pose_optimization_kernel<4>, dim3(n_problems), dim3(256), po_lds, q, (const PoseProbDev *)(base + o_probs));
    else
        hipLaunchKernelGGL(pose_optimization_kernel<0>, dim3(n_problems), dim3(256), po_lds, q, (const PoseProbDev *)(base + o_probs));
    AOS2_HIP_CHECK(hipEventRecord(s->ev[1], q));
    const uint8_t *res = s->h_stage.p;
    AOS2_HIP_CHECK(hipMemcpyAsync(s->h_stage.p, base + o_res, res_bytes, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    (void)hipEventElapsedTime(&s->last_pose_ms, s->ev[0], s->ev[1]);
    for (int i = 0; i < n_problems; ++i) {
        const double *pose = reinterpret_cast<const double *>(res + (offs[i].pose - o_res));
        const int32_t *cnt = reinterpret_cast<const int32_t *>(res + (offs[i].cnt - o_res));
        if (problems[i].n > 0) memcpy(results[i].outlier, res + (offs[i].out - o_res), (size_t)problems[i].n);
        if (problems[i].n < 3)   // the reference returns before touching mTcw (:355-356): keep the caller's matrix bit for bit
            memcpy(results[i].Tcw, problems[i].Tcw, sizeof(float) * 16);
        else
            pose_to_Tcw(pose, results[i].Tcw);
        results[i].n_bad = cnt[0];
        results[i].n_inliers = cnt[1];
    }
    return AOS2_OK;
}


__global__ void debug_pose_blocks_kernel(const double *upd, const double *T, double *T_out, const double *Hb, const double *lambda,
                                        double *x, uint8_t *ok, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double u[6], t[7], xv[6], hb[27];
    for (int k = 0; k < 6; ++k) u[k] = upd[6 * i + k];
    for (int k = 0; k < 7; ++k) t[k] = T[7 * i + k];
    se3_oplus_fast(u, t);
    for (int k = 0; k < 7; ++k) T_out[7 * i + k] = t[k];
    for (int k = 0; k < 27; ++k) hb[k] = Hb[27 * i + k];
    for (int k = 0; k < 6; ++k) xv[k] = x[6 * i + k];
    ok[i] = solve6(hb, lambda[i], xv) ? 1 : 0;
    for (int k = 0; k < 6; ++k) x[6 * i + k] = xv[k];
}

int aos2_debug_pose_blocks_device(const double *upd, const double *T, double *T_out, const double *Hb, const double *lambda,
                                  double *x, uint8_t *ok, int n, int device)
{
    int st;
    if ((st = bind_device(device))) return st;
    DevBuf<double> d;
    DevBuf<uint8_t> dk;
    const size_t N = (size_t)n;
    if ((st = d.alloc(N * (6 + 7 + 7 + 27 + 1 + 6))) || (st = dk.alloc(N))) return st;
    double *du = d.p, *dT = du + 6 * N, *dTo = dT + 7 * N, *dH = dTo + 7 * N, *dl = dH + 27 * N, *dx = dl + N;
    AOS2_HIP_CHECK(hipMemcpy(du, upd, 48 * N, hipMemcpyHostToDevice));
    AOS2_HIP_CHECK(hipMemcpy(dT, T, 56 * N, hipMemcpyHostToDevice));
    AOS2_HIP_CHECK(hipMemcpy(dH, Hb, 216 * N, hipMemcpyHostToDevice));
    AOS2_HIP_CHECK(hipMemcpy(dl, lambda, 8 * N, hipMemcpyHostToDevice));
    AOS2_HIP_CHECK(hipMemcpy(dx, x, 48 * N, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(debug_pose_blocks_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, du, dT, dTo, dH, dl, dx, dk.p, n);
    AOS2_HIP_CHECK(hipDeviceSynchronize());
    AOS2_HIP_CHECK(hipMemcpy(T_out, dTo, 56 * N, hipMemcpyDeviceToHost));
    AOS2_HIP_CHECK(hipMemcpy(x, dx, 48 * N, hipMemcpyDeviceToHost));
    AOS2_HIP_CHECK(hipMemcpy(ok, dk.p, N, hipMemcpyDeviceToHost));
    d.release();
    dk.release();
    return AOS2_OK;
}

}  // extern "C"

// aos2_debug_pose_pass_device: pose_optimization_body in a chosen instantiation, one workgroup per case.  The launch of a form covers all
// cases; a workgroup whose case asked for another form leaves at once.
template <int kForm, int kEpt, int NT, bool kTap>
__global__ __launch_bounds__(NT) void pose_pass_tap_kernel(const PoseProbDev *__restrict__ probs, const PoseTap *__restrict__ taps)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];  // po_lds_bytes(NT)
    __shared__ int s_cnt;
    const PoseTap tap = taps[blockIdx.x];
    if (tap.form != kForm) return;
    const PoseProbDev P = probs[blockIdx.x];
    pose_optimization_body<kEpt, NT, kTap>(P, sh, &s_cnt, &tap);
}

template <bool kTap>
static void pose_pass_tap_launch(int form, int n_cases, const PoseProbDev *probs, const PoseTap *taps)
{
    const dim3 g((unsigned)n_cases);
    if (form == 0) hipLaunchKernelGGL((pose_pass_tap_kernel<0, 4, 256, kTap>), g, dim3(256), po_lds_bytes(256), 0, probs, taps);
    if (form == 1) hipLaunchKernelGGL((pose_pass_tap_kernel<1, 8, 256, kTap>), g, dim3(256), po_lds_bytes(256), 0, probs, taps);
    if (form == 2) hipLaunchKernelGGL((pose_pass_tap_kernel<2, 9, 128, kTap>), g, dim3(128), po_lds_bytes(128), 0, probs, taps);
    if (form == 3) hipLaunchKernelGGL((pose_pass_tap_kernel<3, 0, 256, kTap>), g, dim3(256), po_lds_bytes(256), 0, probs, taps);
}

extern "C" {

int aos2_debug_pose_pass_device(aos2_pose_pass_case_t *cases, int n_cases, int mode, int device)
{
    static const int form_max[4] = {256 * 4, 256 * 8, 128 * 9, INT32_MAX};
    if (!cases || n_cases < 1 || mode < 0 || mode > 2) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n_cases; ++i) {
        const aos2_pose_pass_case_t &c = cases[i];
        if (c.form < 0 || c.form > 3 || c.n < 0 || c.n > form_max[c.form] || c.it < 0 || c.it > 3 || !c.Xw || !c.obs || !c.inv_sigma2 ||
            !c.stereo || !c.level1 || !c.robust || !c.outlier || !c.chi2) {
            set_error("bad pose pass case %d", i);
            return AOS2_ERR_ARG;
        }
    }
    int st;
    if ((st = bind_device(device))) return st;
    // one buffer: per case Xw | obs | w | chi2 | stereo | level1 | robust | outlier (16-byte aligned parts), then the descriptors and results
    struct Off { size_t xw, obs, w, err, st, l1, rb, out; };
    std::vector<Off> offs((size_t)n_cases);
    size_t size = 0;
    auto take = [&](size_t bytes) {
        const size_t o = size;
        size = (size + bytes + 15) & ~(size_t)15;
        return o;
    };
    for (int i = 0; i < n_cases; ++i) {
        const size_t n = (size_t)cases[i].n;
        Off &o = offs[i];
        o.xw = take(12 * n + 4); o.obs = take(12 * n + 4); o.w = take(4 * n + 4); o.err = take(8 * n + 8);
        o.st = take(n + 1); o.l1 = take(n + 1); o.rb = take(n + 1); o.out = take(n + 1);
    }
    const size_t N = (size_t)n_cases;
    const size_t o_probs = take(sizeof(PoseProbDev) * N), o_taps = take(sizeof(PoseTap) * N);
    const size_t o_pose = take(56 * N), o_cnt = take(8 * N), o_sums = take(8 * (size_t)kPoSum * N);
    std::vector<uint8_t> h(size, 0);
    DevBuf<uint8_t> d;
    if ((st = d.alloc(size))) return st;
    uint8_t *base = d.p;
    PoseProbDev *probs = reinterpret_cast<PoseProbDev *>(h.data() + o_probs);
    PoseTap *taps = reinterpret_cast<PoseTap *>(h.data() + o_taps);
    bool used[4] = {false, false, false, false};
    for (int i = 0; i < n_cases; ++i) {
        const aos2_pose_pass_case_t &c = cases[i];
        const size_t n = (size_t)c.n;
        const Off &o = offs[i];
        memcpy(h.data() + o.xw, c.Xw, 12 * n);
        memcpy(h.data() + o.obs, c.obs, 12 * n);
        memcpy(h.data() + o.w, c.inv_sigma2, 4 * n);
        memcpy(h.data() + o.err, c.chi2, 8 * n);
        memcpy(h.data() + o.st, c.stereo, n);
        memcpy(h.data() + o.l1, c.level1, n);
        memcpy(h.data() + o.rb, c.robust, n);
        memcpy(h.data() + o.out, c.outlier, n);
        PoseProbDev &D = probs[i];
        D.n = c.n;
        D.Xw = (const float *)(base + o.xw); D.obs = (const float *)(base + o.obs);
        D.w = (const float *)(base + o.w); D.stereo = base + o.st;
        D.err = (double *)(base + o.err); D.level1 = base + o.l1; D.robust = base + o.rb; D.outlier = base + o.out;
        D.pose_out = (double *)(base + o_pose) + 7 * (size_t)i; D.counts = (int32_t *)(base + o_cnt) + 2 * (size_t)i;
        D.fx = (double)c.fx; D.fy = (double)c.fy; D.cx = (double)c.cx; D.cy = (double)c.cy; D.bf = (double)c.bf;
        for (int k = 0; k < 7; ++k) D.pose_in[k] = c.pose[k];
        taps[i].mode = mode;
        taps[i].it = c.it;
        taps[i].form = c.form;
        taps[i].sums = (double *)(base + o_sums) + (size_t)kPoSum * (size_t)i;
        used[c.form] = true;
    }
    hipError_t e = hipMemcpy(base, h.data(), size, hipMemcpyHostToDevice);
    for (int form = 0; form < 4 && e == hipSuccess; ++form) {
        if (!used[form]) continue;
        if (mode == 0)
            pose_pass_tap_launch<false>(form, n_cases, (const PoseProbDev *)(base + o_probs), (const PoseTap *)(base + o_taps));
        else
            pose_pass_tap_launch<true>(form, n_cases, (const PoseProbDev *)(base + o_probs), (const PoseTap *)(base + o_taps));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h.data(), base, size, hipMemcpyDeviceToHost);
    d.release();
    if (e != hipSuccess) {
        set_error("pose pass tap failed: %s", hipGetErrorString(e));
        return AOS2_ERR_HIP;
    }
    for (int i = 0; i < n_cases; ++i) {
        aos2_pose_pass_case_t &c = cases[i];
        const size_t n = (size_t)c.n;
        const Off &o = offs[i];
        memcpy(c.chi2, h.data() + o.err, 8 * n);
        memcpy(c.level1, h.data() + o.l1, n);
        memcpy(c.robust, h.data() + o.rb, n);
        memcpy(c.outlier, h.data() + o.out, n);
        memcpy(c.sums, h.data() + o_sums + 8 * (size_t)kPoSum * (size_t)i, 8 * (size_t)kPoSum);
        memcpy(c.pose_out, h.data() + o_pose + 56 * (size_t)i, 56);
        const int32_t *cnt = reinterpret_cast<const int32_t *>(h.data() + o_cnt) + 2 * (size_t)i;
        c.n_bad = cnt[0];
        c.n_inliers = cnt[1];
        pose_to_Tcw(c.pose_out, c.Tcw);
    }
    return AOS2_OK;
}

float aos2_pose_optimization_last_device_ms(const aos2_lba_t *s) { return s ? s->last_pose_ms : 0.f; }

}  // extern "C"
